"""Shared case builders of tests/test_update_batch_gpu.py: the problems of a batched update (covariance function, mean
function, old and new observations per problem), their fits on the device and on the oracle, and the C-ABI call."""
import ctypes as C

import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from oracle import oracle_py as orc


class Elevation(ab.ScalingFunction):
    _params = {"elevation_scaling_center": 4.0, "elevation_scaling_factor": 0.3}

    def get_name(self):
        return "elevation_scaling"

    def _call_impl(self, c):
        p = self.get_params()
        return 1. + p["elevation_scaling_factor"] * np.maximum(p["elevation_scaling_center"] - np.asarray(c)[:, 2], 0.)


def covariance(kind, b):
    """(covariance function, mean function or None, dimension) of problem b of a batch of `kind`"""
    if kind in ("fast1", "fast2", "fast3"):  # one radial + noise tree for the whole batch: the one-launch covariance kernels
        return ab.Matern52(1.5 + 0.02 * b, 1.0) + ab.IndependentNoise(0.1 + 0.002 * b), None, int(kind[-1])
    if kind == "mixed":  # two operators in one batch: a launch per problem
        return (ab.Matern52(1.5 + 0.1 * b, 1.0) if b % 2 else ab.SquaredExponential(1.0 + 0.1 * b, 1.2)) + ab.IndependentNoise(0.1), None, 3
    if kind == "update_tree":  # the tree of tests/test_update_dense_gpu.py: update differs from a full fit here
        return (ab.Matern52(2.0 + 0.05 * b, 1.0) + ab.IndependentNoise(0.2) + ab.measurement_only(ab.IndependentNoise(0.3)),
                ab.LinearMean(0.2, -0.5), 3)
    if kind == "dim4":
        return ab.Matern52(2.5 + 0.1 * b, 1.0) + ab.IndependentNoise(0.1), None, 4
    if kind == "scaling":
        return ab.ScalingTerm(Elevation()) * ab.Constant(0.5) + ab.Matern52(2.0 + 0.1 * b, 1.0) + ab.IndependentNoise(0.1), None, 3
    raise ValueError(kind)


class Problem:
    def __init__(self, cov, mean, x, y, var):
        self.cov, self.mean, self.x, self.y, self.var = cov, mean, x, y, var

    def dataset(self, sl):
        targets = self.y[sl] if self.var is None else ab.MarginalDistribution(self.y[sl], self.var[sl])
        return ab.RegressionDataset(self.x[sl], targets)

    def model(self, ctx):
        if self.mean is None:
            return ab.gp_from_covariance(self.cov, context=ctx)
        return ab.gp_from_covariance_and_mean(self.cov, self.mean, context=ctx)

    def oracle(self, sl):
        return orc.OracleFit(self.cov, self.x[sl], self.y[sl], None if self.var is None else self.var[sl], mean=self.mean)

    def oracle_update(self, of, sl):
        return of.update(self.x[sl], self.y[sl], None if self.var is None else self.var[sl])


def problems(kind, n, count, seed, with_variance, duplicate_at=None):
    """`count` problems of `kind` with n observations each; duplicate_at = (i, j): observation i lies AT observation j"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(count):
        cov, mean, dim = covariance(kind, b)
        x = rng.uniform(0., 10., (n, dim))
        if duplicate_at:
            x[duplicate_at[0]] = x[duplicate_at[1]]
        y = np.sin(x).sum(axis=1) + 0.05 * rng.standard_normal(n) + 0.05 * b
        out.append(Problem(cov, mean, x, y, rng.uniform(0.05, 0.1, n) if with_variance else None))
    return out


def fit_old(ctx, probs, n0, origin="batch"):
    """FitModels of the first n0 observations: origin "batch" = one fit_batch call; "mixed" = all but the last from one
    fit_batch call and the last from fit() (an allocation of its own: no constant stride)"""
    models = [p.model(ctx) for p in probs]
    datasets = [p.dataset(slice(0, n0)) for p in probs]
    if origin == "batch":
        return models, ab.fit_batch(models, datasets)
    return models, ab.fit_batch(models[:-1], datasets[:-1]) + [models[-1].fit(datasets[-1])]


def block_matrix(p, n0, n):
    """the matrix whose LL^T the grown factor is: the old Gram matrix on measurements, cross and new block on plain features"""
    a, b = slice(0, n0), slice(n0, n)
    var = np.zeros(n) if p.var is None else p.var
    K = orc.gram(p.cov, p.x[a], x_meas=True) + np.diag(var[a])
    return np.block([[K, orc.gram(p.cov, p.x[a], p.x[b])], [orc.gram(p.cov, p.x[b], p.x[a]), orc.gram(p.cov, p.x[b]) + np.diag(var[b])]])


def _to_device(ctx, a):
    """a copy of a's MEMORY in HBM (Context.to_device takes the C-ordered values: hand it the transpose of a column-major array)"""
    return ctx.to_device(a.T if (a.flags.f_contiguous and not a.flags.c_contiguous) else np.ascontiguousarray(a))


class CapiCall:
    """one agp_fit_update_batch call at the C-ABI level: new features and targets in host memory or resident in HBM"""

    def __init__(self, ctx, models, fms, probs, sl, where="host", information=True):
        self.ctx, self.count = ctx, len(fms)
        self.fsets = [m.covariance_function_.features(p.x[sl]) for m, p in zip(models, probs)]
        self.m = self.fsets[0].n
        ys = [m._targets(fs, p.dataset(sl).targets) for m, fs, p in zip(models, self.fsets, probs)]
        self.Y = np.asfortranarray(np.stack([y for y, _ in ys], axis=1))
        self.V = None if ys[0][1] is None else np.asfortranarray(np.stack([v for _, v in ys], axis=1))
        self.keep = []
        self.structs = []
        for fs in self.fsets:
            s = fs.as_struct()
            if where == "device":
                for field, a in (("coords", fs.coords), ("eq_id", fs.eq_id), ("scales", fs.scales)):
                    if a is not None:
                        d = _to_device(ctx, a)
                        self.keep.append(d)
                        setattr(s, field, d.ptr)
                s.location = capi.DEVICE
            self.structs.append(s)
        self.y_ptr, self.v_ptr = abgp._ptr(self.Y), (None if self.V is None else abgp._ptr(self.V))
        if where == "device":
            dy = _to_device(ctx, self.Y)
            self.keep.append(dy)
            self.y_ptr = C.c_void_p(dy.ptr)
            if self.V is not None:
                dv = _to_device(ctx, self.V)
                self.keep.append(dv)
                self.v_ptr = C.c_void_p(dv.ptr)
        self.kernels = [ctx.private_kernel(m.covariance_function_) for m in models]
        self.olds = [fm.get_fit()._h.value for fm in fms]
        self.rows = fms[0].get_fit().rows() + self.m
        self.information = np.full((self.rows, self.count), -7.0, order="F") if information else None
        self.log_det = np.full(self.count, -7.0)
        self.status = (C.c_int * self.count)(*([-99] * self.count))
        self.out = (C.c_void_p * self.count)(*([0xdead] * self.count))

    def run(self, count=None, olds=None, ldi=None):
        count = self.count if count is None else count
        olds = self.olds if olds is None else olds
        rc = self.ctx._lib.agp_fit_update_batch(
            self.ctx._h, count, (C.c_void_p * self.count)(*self.kernels), (C.c_void_p * self.count)(*olds),
            (C.c_void_p * self.count)(*[C.addressof(s) for s in self.structs]), self.y_ptr, self.m, self.v_ptr, self.m, self.out,
            None if self.information is None else abgp._ptr(self.information), self.rows if ldi is None else ldi,
            abgp._ptr(self.log_det), self.status)
        return rc

    def fits(self):
        """the published handles as GPFits (which destroy them)"""
        return [abgp.GPFit(self.ctx, C.c_void_p(self.out[b]), self.rows, None) for b in range(self.count)]

    def close(self):
        for k in self.kernels:
            self.ctx._lib.agp_kernel_destroy(k)
        self.kernels = []
