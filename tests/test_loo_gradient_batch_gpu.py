"""GPU tests of agp_loo_nll_gradient_batch: GaussianProcessRegression.leave_one_out_likelihoods / _gradients (parameter
vectors of one model) and ab.leave_one_out_likelihood_gradient_batch (independent models), the C-ABI's per-problem
status and argument checks, and the batched G^T G kernel on its own.

Reference values: the numpy closed form of test_loo_gradient_gpu.py (`reference`, itself checked against brute-force
refits there), with that file's tolerances: the value to 1e-10 relative, |g - g_ref| <= 1e-7 s_p with its s_p, the sum
of the magnitudes of the terms the gradient adds up.  Against the single call (agp_loo_nll_gradient): 1e-9 s_p for the
gradient and 1e-10 relative for the value, the batch-against-single bound of test_nll_gradient_batch_gpu.py - the
batched and the single factorisations differ in their schedule, and u_b = C_b a_b is summed in another order.  The
value-only path against the full one: 1e-12 relative (c_i from R's column norms against R^T R's diagonal).

Factor paths, as test_nll_gradient_batch_gpu.py documents them: n = 64 is one 128-block, n = 300 / 512 run the fused
panels, n = 1100 with 64 problems takes the two-stream look-ahead schedule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from conftest import synthetic_3d
from test_loo_gradient_gpu import _dataset, _variance, reference
from test_nll_gradient_batch_gpu import _config3, _copy, _heterogeneous, _numpy_subset, _p, _sets
from test_nll_gradient_gpu import _elevation_model, _FirstCoordinateMean, _padded_data

pytestmark = pytest.mark.gpu


def _check_numpy(model, x, y, s, value, grad):
    want, scale, ref_value, _ = reference(model, x, y, s)
    assert set(grad) == set(want)
    assert abs(value - ref_value) <= 1e-10 * abs(ref_value), (value, ref_value)
    for name in want:
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    return scale


def _check_single(model, ds, value, grad, scale):
    v1, g1 = model.leave_one_out_likelihood_gradient(ds)
    assert abs(value - v1) <= 1e-10 * abs(v1), (value, v1)
    for name in g1:
        assert abs(grad[name] - g1[name]) <= 1e-9 * scale[name], (name, grad[name], g1[name], scale[name])


SIZES = [64, 300, 512, 1100]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("count", [1, 3, 8, 64])
def test_config3_matches_numpy_single_and_value_only(ctx, count, n):
    x, y = synthetic_3d(n, 7 + n)
    s = _variance(n, n) if SIZES.index(n) % 2 == 1 else None  # with a target variance at n = 300 and 1100
    model = _config3(ctx)
    ds = _dataset(x, y, s)
    sets = _sets(model, count, count * 1000 + n)
    values, grads = model.leave_one_out_likelihood_gradients(ds, sets)
    assert values.shape == (count,) and len(grads) == count
    only = model.leave_one_out_likelihoods(ds, sets)  # the value-only path
    assert only.shape == (count,)
    for b in range(count):
        assert abs(values[b] - only[b]) <= 1e-12 * abs(values[b]), (b, values[b], only[b])
    for b in _numpy_subset(count):
        m = _copy(model, sets[b])
        scale = _check_numpy(m, x, y, s, values[b], grads[b])
        if b in (0, count - 1):
            _check_single(m, ds, values[b], grads[b], scale)


@pytest.mark.parametrize("count,n", [(3, 300), (8, 1100)])
def test_elevation_model_with_a_variance_per_problem(ctx, count, n):
    """ScalingTerm, Constant, Matern52, noise and a linear mean; every problem has its own parameters, tangent columns
    and target variance (ldv = n)"""
    rng = np.random.default_rng(n)
    x = rng.uniform(0., 10., (n, 3))
    y = np.sin(x).sum(axis=1) + 0.3 * x[:, 0]
    _, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    models = [_copy(model, o) for o in _sets(model, count, n, spread=0.2)]
    variances = [_variance(n, 100 + b) for b in range(count)]
    datasets = [_dataset(x, y, s) for s in variances]
    out = ab.leave_one_out_likelihood_gradient_batch(models, datasets)
    assert len(out) == count
    for m, s, ds, (value, grad) in zip(models, variances, datasets, out):
        assert {"elevation_scaling_center", "elevation_scaling_factor", "slope", "offset"} <= set(grad)
        scale = _check_numpy(m, x, y, s, value, grad)
        _check_single(m, ds, value, grad, scale)


def _heterogeneous_datasets(ctx, n):
    """_heterogeneous's six models (1-D, 2-D and 3-D, 1 to 9 slots), every second one with a target variance"""
    problems = _heterogeneous(ctx, n)
    variances = [_variance(n, 40 + b) if b % 2 else None for b in range(len(problems))]
    return problems, variances, [_dataset(x, y, s) for (_, x, y), s in zip(problems, variances)]


def test_heterogeneous_batch_matches_numpy_and_single_calls(ctx):
    n = 300
    problems, variances, datasets = _heterogeneous_datasets(ctx, n)
    out = ab.leave_one_out_likelihood_gradient_batch([m for m, _, _ in problems], datasets)
    assert len(out) == len(problems)
    for (m, x, y), s, ds, (value, grad) in zip(problems, variances, datasets, out):
        assert set(grad) == set(m.get_params())
        scale = _check_numpy(m, x, y, s, value, grad)
        _check_single(m, ds, value, grad, scale)


def test_batch_of_dimensions_2_4_5(ctx):
    """One launch on Point<8> for problems of 2, 4 and 5 dimensions.  n = 130: full and partial tiles of the
    64-contraction and of the 32-tile G kernel."""
    problems, variances = [], []
    for dim in (2, 4, 5):
        model = ab.gp_from_covariance(ab.SquaredExponential(1.5, 1.2) + ab.IndependentNoise(0.1), context=ctx)
        problems.append((model, *_padded_data(dim)))
        variances.append(_variance(130, dim))
    datasets = [_dataset(x, y, s) for (_, x, y), s in zip(problems, variances)]
    out = ab.leave_one_out_likelihood_gradient_batch([m for m, _, _ in problems], datasets)
    for (m, x, y), s, ds, (value, grad) in zip(problems, variances, datasets, out):
        scale = _check_numpy(m, x, y, s, value, grad)
        _check_single(m, ds, value, grad, scale)


def _bits(results):
    return [(np.float64(v).tobytes(), tuple(sorted((k, np.float64(g).tobytes()) for k, g in grad.items()))) for v, grad in results]


def test_deterministic_and_permutation_invariant(ctx):
    problems, _, datasets = _heterogeneous_datasets(ctx, 300)
    models = [m for m, _, _ in problems]
    first = _bits(ab.leave_one_out_likelihood_gradient_batch(models, datasets))
    assert _bits(ab.leave_one_out_likelihood_gradient_batch(models, datasets)) == first
    rev = _bits(ab.leave_one_out_likelihood_gradient_batch(models[::-1], datasets[::-1]))
    assert rev[::-1] == first


def test_result_does_not_depend_on_the_neighbours(ctx):
    """problem 0 in two batches of the same count whose other problems differ (same trees and dimension)"""
    x, y = synthetic_3d(512, 3)
    model = _config3(ctx)
    ds = _dataset(x, y, _variance(512, 6))
    mine = {"sigma_squared_exponential": 1.3}
    a = model.leave_one_out_likelihood_gradients(ds, [mine] + _sets(model, 8, 1)[1:])
    b = model.leave_one_out_likelihood_gradients(ds, [mine] + _sets(model, 8, 2)[1:])
    assert np.float64(a[0][0]).tobytes() == np.float64(b[0][0]).tobytes()
    assert all(np.float64(a[1][0][k]).tobytes() == np.float64(b[1][0][k]).tobytes() for k in a[1][0])
    va = model.leave_one_out_likelihoods(ds, [mine] + _sets(model, 8, 1)[1:])
    vb = model.leave_one_out_likelihoods(ds, [mine] + _sets(model, 8, 2)[1:])
    assert va[0].tobytes() == vb[0].tobytes()


# ---- the C-ABI directly -------------------------------------------------------------------------------------------
class _Raw:
    """the arguments of one agp_loo_nll_gradient_batch call, built from (model, x, y, s) problems (s: the target variance
    or None - then zeros beside problems that have one), with every array kept alive"""

    def __init__(self, ctx, problems):
        self.ctx = ctx
        self.models = [p[0] for p in problems]
        self.probs = [abgp._gradient_problem(m, _dataset(x, y, s)) for m, x, y, s in problems]
        self.count = len(problems)
        self.n = self.probs[0].fs.n
        self.structs = [p.fs.as_struct() for p in self.probs]
        self.Y = np.asfortranarray(np.stack([p.y for p in self.probs], axis=1))
        self.V = None
        if any(p.yv is not None for p in self.probs):
            self.V = np.asfortranarray(np.stack([np.zeros(self.n) if p.yv is None else p.yv for p in self.probs], axis=1))
        self.ldg = max(1, max(len(p.slots) for p in self.probs))
        self.n_slots = (C.c_int * self.count)(*[len(p.slots) for p in self.probs])
        self.tables = (C.c_void_p * self.count)(*[C.addressof(p.table) for p in self.probs])
        self.tang = (C.c_void_p * self.count)(*[None if p.tangents is None else p.tangents.ctypes.data for p in self.probs])

    def call(self, weights=True, **over):
        """(rc, loo, grad, mean_weights, status), the outputs sentinel-filled before the call"""
        ctx = self.ctx
        loo = np.full(self.count, 7.0)
        grad = np.full((self.count, self.ldg), 7.0)
        u = np.full((self.count, self.n), 7.0)
        status = (C.c_int * self.count)(*([-5] * self.count))
        handles = [ctx.private_kernel(m.covariance_function_) for m in self.models]
        try:
            kernels = (C.c_void_p * self.count)(*handles)
            fptrs = (C.c_void_p * self.count)(*[C.addressof(s) for s in self.structs])
            rc = ctx._lib.agp_loo_nll_gradient_batch(
                ctx._h, over.get("count", self.count), kernels, fptrs, over.get("y", _p(self.Y)), over.get("ldy", self.n),
                over.get("y_var", None if self.V is None else _p(self.V)), over.get("ldv", self.n),
                over.get("n_slots", self.n_slots), over.get("slots", self.tables), over.get("tangents", self.tang),
                over.get("ldt", self.n), _p(loo), _p(grad), over.get("ldg", self.ldg), _p(u) if weights else None,
                over.get("ldw", self.n), status)
        finally:
            for h in handles:
                ctx._lib.agp_kernel_destroy(h)
        return rc, loo, grad, u, list(status)

    def gradient_dict(self, b, grad, u):
        return self.models[b]._leave_one_out_gradient_dict(self.probs[b].slots, grad[b, :self.n_slots[b]], u[b], self.probs[b].fs)


def test_a_problem_without_slots_beside_problems_with_slots(ctx):
    """n_slots[b] = 0 for one problem of the heterogeneous batch: its value and mean weights keep their bits, its
    gradient column is not written, and the other problems keep theirs"""
    problems, variances, _ = _heterogeneous_datasets(ctx, 300)
    raw = _Raw(ctx, [(m, x, y, s) for (m, x, y), s in zip(problems, variances)])
    full = raw.call()
    assert full[0] == capi.AGP_OK and full[4] == [0] * raw.count
    n_slots = (C.c_int * raw.count)(*raw.n_slots)
    n_slots[4] = 0  # the nine-slot problem: the batch keeps two slot groups, the largest problem leaves
    part = raw.call(n_slots=n_slots)
    assert part[0] == capi.AGP_OK and part[4] == [0] * raw.count
    assert part[1].tobytes() == full[1].tobytes() and part[3].tobytes() == full[3].tobytes()
    assert (part[2][4] == 7.0).all()
    for b in (0, 1, 2, 3, 5):
        assert part[2][b, :raw.n_slots[b]].tobytes() == full[2][b, :raw.n_slots[b]].tobytes(), b
    m, x, y = problems[4]
    value = reference(m, x, y, variances[4])[2]
    assert abs(part[1][4] - value) <= 1e-10 * abs(value)


def test_shared_vectors_give_the_bits_of_replicated_ones(ctx):
    """ldy = 0 and ldv = 0: one y and one y_var for every problem"""
    n = 300
    x, y = synthetic_3d(n, 5)
    s = _variance(n, 8)
    model = _config3(ctx)
    raw = _Raw(ctx, [(_copy(model, o), x, y, s) for o in _sets(model, 4, 21)])
    rep = raw.call()
    assert rep[0] == capi.AGP_OK and rep[4] == [0, 0, 0, 0]
    y1, s1 = np.ascontiguousarray(y), np.ascontiguousarray(s)
    one = raw.call(y=_p(y1), ldy=0, y_var=_p(s1), ldv=0)
    assert one[0] == capi.AGP_OK and one[4] == [0, 0, 0, 0]
    for a, b in zip(rep[1:4], one[1:4]):
        assert a.tobytes() == b.tobytes()
    only_rep, only_one = raw.call(weights=False, n_slots=(C.c_int * 4)()), raw.call(weights=False, n_slots=(C.c_int * 4)(), y=_p(y1),
                                                                                      ldy=0, y_var=_p(s1), ldv=0)
    assert only_rep[0] == capi.AGP_OK and only_rep[1].tobytes() == only_one[1].tobytes()


def test_failed_problems_are_reported_and_isolated(ctx):
    n = 300
    rng = np.random.default_rng(4)
    problems = []
    for b in range(6):
        x = rng.uniform(0., 10., (n, 3))
        problems.append((_config3(ctx), x, np.sin(x).sum(axis=1), None))
    xs = problems[1][1].copy()
    xs[5] = xs[0]  # no noise + a duplicated point: singular
    problems[1] = (ab.gp_from_covariance(ab.SquaredExponential(1., 1.), context=ctx), xs, problems[1][2], None)
    xn = problems[4][1].copy()
    xn[17, 1] = np.nan
    problems[4] = (problems[4][0], xn, problems[4][2], None)
    raw = _Raw(ctx, problems)
    rc, loo, grad, u, status = raw.call()
    assert rc == capi.AGP_OK
    assert status[1] == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and status[4] == capi.AGP_ERR_NAN_INPUT
    for b in (1, 4):
        assert np.isnan(loo[b]) and np.isnan(grad[b, :raw.n_slots[b]]).all()
        assert (u[b] == 7.0).all()  # left untouched
    for b in (0, 2, 3, 5):
        assert status[b] == capi.AGP_OK
        m, x, y, _ = problems[b]
        scale = reference(m, x, y, None)[1]
        _check_single(m, ab.RegressionDataset(x, y), loo[b], raw.gradient_dict(b, grad, u), scale)
    # the value-only path reports the same
    rc, only, _, _, status = raw.call(weights=False, n_slots=(C.c_int * 6)())
    assert rc == capi.AGP_OK and status[1] == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and status[4] == capi.AGP_ERR_NAN_INPUT
    assert np.isnan(only[[1, 4]]).all()
    for b in (0, 2, 3, 5):
        assert abs(only[b] - loo[b]) <= 1e-12 * abs(loo[b])
    # the Python layers give NaN, not an exception
    out = ab.leave_one_out_likelihood_gradient_batch([p[0] for p in problems], [ab.RegressionDataset(p[1], p[2]) for p in problems])
    assert np.isnan(out[1][0]) and all(np.isnan(v) for v in out[4][1].values())
    assert not np.isnan(out[0][0])


def test_not_positive_definite_set_gives_nan(ctx):
    rng = np.random.default_rng(8)
    x = rng.uniform(0., 10., (200, 3))
    x[1] = x[0]  # without noise: K_00 = K_01 = K_11 = 1 exactly, the second pivot is 0
    model = _config3(ctx)
    ds = ab.RegressionDataset(x, np.sin(x).sum(axis=1))
    sets = [{}, {"sigma_independent_noise": 0.0}, {"sigma_squared_exponential": 1.2}]
    values, grads = model.leave_one_out_likelihood_gradients(ds, sets)
    assert np.isnan(values[1]) and all(np.isnan(v) for v in grads[1].values())
    assert not np.isnan(values[0]) and not np.isnan(values[2])
    only = model.leave_one_out_likelihoods(ds, sets)
    assert np.isnan(only[1]) and not np.isnan(only[0]) and not np.isnan(only[2])


def test_argument_errors_write_nothing(ctx):
    n = 100
    rng = np.random.default_rng(2)
    x = rng.uniform(0., 10., (n, 3))
    _, elev = _elevation_model(ctx)
    problems = [(_config3(ctx), x, np.sin(x).sum(axis=1), None), (elev, x, np.cos(x).sum(axis=1), None)]
    raw = _Raw(ctx, problems)
    rc, loo, grad, u, status = raw.call()
    assert rc == capi.AGP_OK and status == [0, 0]

    def untouched(res, over):
        rc, loo, grad, u, status = res
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT, over
        assert (loo == 7.0).all() and (grad == 7.0).all() and (u == 7.0).all() and status == [-5, -5], over

    def rejected(**over):
        untouched(raw.call(**over), over)

    rejected(count=0)
    rejected(count=-1)
    rejected(ldy=n - 1)
    rejected(ldg=raw.ldg - 1)
    rejected(ldw=n - 1)
    assert raw.call(weights=False, ldw=n - 1)[0] == capi.AGP_OK  # ldw is not read without mean_weights
    rejected(ldt=n - 1)
    rejected(tangents=None)
    rejected(tangents=(C.c_void_p * 2)(raw.tang[0], None))
    rejected(n_slots=(C.c_int * 2)(raw.n_slots[0], capi.MAX_GRADIENT_SLOTS + 1))
    rejected(n_slots=(C.c_int * 2)(-1, raw.n_slots[1]))
    bad = (capi.GradientSlot * 1)(capi.GradientSlot(2, 0))  # the sum node of SE + noise
    rejected(slots=(C.c_void_p * 2)(C.addressof(bad), raw.tables[1]), n_slots=(C.c_int * 2)(1, raw.n_slots[1]))
    rejected(slots=(C.c_void_p * 2)(None, raw.tables[1]))
    rejected(slots=None)
    # n mismatch and mixed locations
    raw2 = _Raw(ctx, problems)
    raw2.structs[1].n = n - 1
    untouched(raw2.call(), "n mismatch")
    raw3 = _Raw(ctx, problems)
    raw3.structs[1].location = capi.DEVICE
    untouched(raw3.call(), "mixed locations")


def test_device_resident_inputs_give_the_same_bits(ctx):
    n = 300
    rng = np.random.default_rng(12)
    x = rng.uniform(0., 10., (n, 3))
    _, elev = _elevation_model(ctx)
    problems = [(elev, x, np.sin(x).sum(axis=1), _variance(n, 1)),
                (_copy(elev, {"elevation_scaling_center": 6.0}), x, np.cos(x).sum(axis=1), _variance(n, 2)),
                (_config3(ctx), x, np.sin(x[:, 0]), _variance(n, 3))]
    raw = _Raw(ctx, problems)
    host = raw.call()
    assert host[0] == capi.AGP_OK and host[4] == [0, 0, 0]

    def dev(a):  # a device copy with the host array's memory layout
        return ctx.to_device(np.ravel(a, order="K"))

    keep = []
    for s, p in zip(raw.structs, raw.probs):
        d = dev(p.fs.coords)
        keep.append(d)
        s.coords = d.ptr
        if p.fs.scales is not None:
            ds_ = dev(p.fs.scales)
            keep.append(ds_)
            s.scales = ds_.ptr
        s.location = capi.DEVICE
    yd, vd = dev(raw.Y), dev(raw.V)
    tang = []
    for p in raw.probs:
        if p.tangents is None:
            tang.append(None)
        else:
            td = dev(p.tangents)
            keep.append(td)
            tang.append(td.ptr)
    res = raw.call(y=C.c_void_p(yd.ptr), y_var=C.c_void_p(vd.ptr), tangents=(C.c_void_p * 3)(*tang))
    assert res[0] == capi.AGP_OK and res[4] == [0, 0, 0]
    for h, d in zip(host[1:4], res[1:4]):
        assert h.tobytes() == d.tobytes()
    for d in keep + [yd, vd]:
        d.free()


# ---- the batched G^T G kernel alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128, 300, 512])
@pytest.mark.parametrize("count", [1, 5, 64])
def test_batched_gtg_kernel_matches_numpy(ctx, count, n):
    dbg = capi.load_debug()
    dbg.agp_debug_gtg_lower_batched.restype = C.c_int
    dbg.agp_debug_gtg_lower_batched.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                C.POINTER(C.c_double)]
    rng = np.random.default_rng(count * 1000 + n)
    ld = n + 8
    Gs = rng.uniform(-1., 1., (count, n, n)) / np.sqrt(n)
    Gd = np.full((count, n, ld), np.nan)  # slab b: column-major ld x n = row-major n x ld; the padding rows must not be read
    Gd[:, :, :n] = Gs.transpose(0, 2, 1)
    Sd = np.zeros_like(Gd)
    ms = C.c_double()
    assert dbg.agp_debug_gtg_lower_batched(ctx._h, _p(Gd), n, ld, count, _p(Sd), C.byref(ms)) == 0
    low = np.tril_indices(n)
    want = Gs.transpose(0, 2, 1) @ Gs
    for b in range(count):
        got = Sd[b, :, :n].T
        assert np.abs(got[low] - want[b][low]).max() <= 1e-13 * np.abs(want[b]).max(), b
    assert np.all(Sd[:, :, n:] == 0.)  # nothing written below row n
    if count == 1:
        dbg.agp_debug_gtg_lower.restype = C.c_int
        dbg.agp_debug_gtg_lower.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_double)]
        S1 = np.zeros_like(Gd)
        assert dbg.agp_debug_gtg_lower(ctx._h, _p(Gd), n, ld, _p(S1), C.byref(ms)) == 0
        assert Sd[0, :, :n].T[low].tobytes() == S1[0, :, :n].T[low].tobytes()


def test_cpp_gradients_match_python(ctx):
    """examples/loo_gradient_batch_check (GaussianProcessRegression::leave_one_out_likelihood_gradients and
    leave_one_out_likelihoods) against the Python batch"""
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "loo_gradient_batch_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y, s = data[:, 1:4], data[:, 4], data[:, 5]
    cov, _ = _elevation_model(ctx)
    model = ab.gp_from_covariance_and_mean(cov, _FirstCoordinateMean(0.2, -0.4), context=ctx)
    sets = [{}, {"elevation_scaling_center": 5.0}, {"sigma_matern_52": 1.3, "slope": 0.5},
            {"elevation_scaling_factor": 0.5, "sigma_independent_noise": 0.2, "offset": 0.1}]
    values, grads = model.leave_one_out_likelihood_gradients(_dataset(x, y, s), sets)
    cpp_value = {int(b): float(v) for b, v in rows["loo_nll"]}
    cpp_only = {int(b): float(v) for b, v in rows["loo_nll_value_only"]}
    assert sorted(cpp_value) == sorted(cpp_only) == list(range(len(sets)))
    for b in range(len(sets)):
        assert abs(cpp_value[b] - values[b]) <= 1e-10 * abs(values[b])
        assert abs(cpp_only[b] - values[b]) <= 1e-10 * abs(values[b])
        cpp = {k[len("grad_"):]: float(v) for k, vs in rows.items() if k.startswith("grad_") for bb, v in vs if int(bb) == b}
        assert set(cpp) == set(grads[b])
        big = max(abs(g) for g in grads[b].values())
        for name, g in grads[b].items():
            assert abs(cpp[name] - g) <= 1e-10 * max(abs(g), 1e-3 * big), (b, name)


def test_repeated_calls_return_device_memory(ctx):
    import gc
    import torch
    problems, _, datasets = _heterogeneous_datasets(ctx, 300)
    models = [m for m, _, _ in problems]
    x, y = synthetic_3d(512, 9)
    model = _config3(ctx)
    ds = ab.RegressionDataset(x, y)

    def cycle():
        ab.leave_one_out_likelihood_gradient_batch(models, datasets)
        model.leave_one_out_likelihood_gradients(ds, _sets(model, 16, 4))
        model.leave_one_out_likelihoods(ds, _sets(model, 16, 4))

    def used():
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2 ** 20

    cycle(); cycle()
    ctx.synchronize(); torch.cuda.synchronize()
    base = used()
    for _ in range(20):
        cycle()
    ctx.synchronize(); torch.cuda.synchronize()
    gc.collect()
    assert used() - base < 64.0
