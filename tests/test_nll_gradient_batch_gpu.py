"""GPU tests of agp_nll_gradient_batch: GaussianProcessRegression.log_likelihood_gradients (parameter vectors of one model)
and ab.log_likelihood_gradient_batch (independent models), the C-ABI's per-problem status and argument checks, and the
batched R^T R kernel on its own.

Reference values: numpy on the oracle's Gram matrices with central differences of dK (reference_gradient of
test_nll_gradient_gpu.py, same tolerance: |g - g_ref| <= 1e-7 s_p, s_p the non-cancelling scale of the summed terms).
Against the single call (agp_nll_gradient): 1e-9 s_p - the batched and the single factorisations differ in their
schedule, both are exact to fp64 rounding at cond(K) <= 1e6.

Factor paths: n = 64 is one 128-block (no fused panel launches: batched_fused_fits is false), n = 300 / 512 batches of
up to 64 problems fit on the chip at once (fused panels), n = 1100 with 64 problems takes the two-stream look-ahead
schedule (count n^2 >= 6e7)."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from conftest import synthetic_3d
from test_nll_gradient_gpu import _FirstCoordinateMean, _elevation_model, _padded_data, reference_gradient

pytestmark = pytest.mark.gpu


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _config3(ctx):
    return ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)


def _sets(model, count, seed, spread=0.3):
    """`count` override dicts: every parameter scaled by a factor in [1 - spread, 1 + spread]; the first is the model"""
    rng = np.random.default_rng(seed)
    base = model.get_params()
    out = [{}]
    for _ in range(count - 1):
        out.append({k: v * (1. + spread * rng.uniform(-1., 1.)) if v != 0. else v + 0.1 * rng.uniform(-1., 1.)
                    for k, v in base.items()})
    return out[:count]


def _copy(model, overrides):
    return model._override_copies([overrides])[0]


def _check_numpy(model, x, y, ll, grad):
    want, scale, ll_ref = reference_gradient(model, x, y)
    assert set(grad) == set(want)
    for name in want:
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    assert abs(ll - ll_ref) <= 1e-8 * len(y)
    return scale


def _check_single(model, ds, ll, grad, scale):
    ll1, g1 = model.log_likelihood_gradient(ds)
    for name in g1:
        assert abs(grad[name] - g1[name]) <= 1e-9 * scale[name], (name, grad[name], g1[name], scale[name])
    assert abs(ll - ll1) <= 1e-10 * max(1., abs(ll))
    assert abs(ll - model.log_likelihood(ds)) <= 1e-10 * max(1., abs(ll))


def _numpy_subset(count):
    """the problems checked against numpy: all of them up to 8, else 8 spread over the batch (first and last included)"""
    return list(range(count)) if count <= 8 else sorted(set(np.linspace(0, count - 1, 8).round().astype(int).tolist()))


@pytest.mark.parametrize("n", [64, 300, 512, 1100])
@pytest.mark.parametrize("count", [1, 3, 8, 64])
def test_config3_gradients_match_numpy(ctx, count, n):
    x, y = synthetic_3d(n, 7 + n)
    model = _config3(ctx)
    ds = ab.RegressionDataset(x, y)
    sets = _sets(model, count, count * 1000 + n)
    lls, grads = model.log_likelihood_gradients(ds, sets)
    assert lls.shape == (count,) and len(grads) == count
    lls_fd = model.log_likelihoods(ds, sets)
    for b in range(count):
        assert abs(lls[b] - lls_fd[b]) <= 1e-10 * max(1., abs(lls[b]))
    for b in _numpy_subset(count):
        m = _copy(model, sets[b])
        scale = _check_numpy(m, x, y, lls[b], grads[b])
        if b in (0, count - 1):
            _check_single(m, ds, lls[b], grads[b], scale)


@pytest.mark.parametrize("count,n", [(3, 300), (8, 512), (8, 1100)])
def test_scaling_term_and_linear_mean_gradients_match_numpy(ctx, count, n):
    """ScalingTerm parameters change the scale columns per problem: every copy gets its own tangents and features"""
    rng = np.random.default_rng(n)
    x = rng.uniform(0., 10., (n, 3))
    y = np.sin(x).sum(axis=1) + 0.3 * x[:, 0]
    _, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    ds = ab.RegressionDataset(x, y)
    sets = _sets(model, count, n, spread=0.2)
    lls, grads = model.log_likelihood_gradients(ds, sets)
    for b in range(count):
        m = _copy(model, sets[b])
        scale = _check_numpy(m, x, y, lls[b], grads[b])
        _check_single(m, ds, lls[b], grads[b], scale)


def test_polynomial_1d_gradients_match_numpy(ctx):
    rng = np.random.default_rng(5)
    n = 300
    x = rng.uniform(-1., 1., n)
    y = 1. + 0.5 * x - x * x + 0.05 * rng.standard_normal(n)
    model = ab.gp_from_covariance(ab.Polynomial(2, 0.8) + ab.SquaredExponential(0.5, 0.3) + ab.IndependentNoise(0.1), context=ctx)
    ds = ab.RegressionDataset(x, y)
    sets = _sets(model, 8, 17, spread=0.2)
    lls, grads = model.log_likelihood_gradients(ds, sets)
    for b in range(8):
        m = _copy(model, sets[b])
        scale = _check_numpy(m, x, y, lls[b], grads[b])
        _check_single(m, ds, lls[b], grads[b], scale)


def _heterogeneous(ctx, n):
    """models with different trees, dimensions (1-D and 3-D) and slot counts (1 ... 9: one to three slot groups), each
    on a dataset of its own"""
    rng = np.random.default_rng(n)
    problems = []
    x3 = rng.uniform(0., 10., (n, 3))
    problems.append((_config3(ctx), x3, np.sin(x3).sum(axis=1)))                                          # P = 3
    x3b = rng.uniform(0., 10., (n, 3))
    _, elev = _elevation_model(ctx)
    elev.set_param_values({"slope": 0.2, "offset": -0.4})
    problems.append((elev, x3b, np.sin(x3b).sum(axis=1) + 0.3 * x3b[:, 0]))                                # P = 6 (+ 2 mean)
    x1 = rng.uniform(-1., 1., n)
    poly = ab.Polynomial(2, 0.8) + ab.SquaredExponential(0.5, 0.3) + ab.IndependentNoise(0.1)
    problems.append((ab.gp_from_covariance(poly, context=ctx), x1, 1. + 0.5 * x1 - x1 * x1))                # P = 6, 1-D
    problems.append((ab.gp_from_covariance(ab.IndependentNoise(0.7), context=ctx), x1, rng.standard_normal(n)))  # P = 1
    x1b = rng.uniform(0., 5., n)
    many = (ab.SquaredExponential(1.5, 1.2) + ab.Matern32(2.5, 0.5) + ab.Matern52(1.0, 0.4) + ab.Exponential(3.0, 0.3)
            + ab.IndependentNoise(0.2))
    problems.append((ab.gp_from_covariance(many, context=ctx), x1b, np.sin(x1b)))                           # P = 9
    x2 = rng.uniform(0., 10., (n, 2))
    m32 = ab.Matern32(2.0, 1.0) * ab.Constant(0.6) + ab.IndependentNoise(0.15)
    problems.append((ab.gp_from_covariance(m32, context=ctx), x2, np.cos(x2).sum(axis=1)))                  # P = 4, 2-D
    return problems


def test_heterogeneous_batch_matches_numpy_and_single_calls(ctx):
    n = 300
    problems = _heterogeneous(ctx, n)
    models = [m for m, _, _ in problems]
    datasets = [ab.RegressionDataset(x, y) for _, x, y in problems]
    out = ab.log_likelihood_gradient_batch(models, datasets)
    assert len(out) == len(problems)
    for (m, x, y), ds, (ll, grad) in zip(problems, datasets, out):
        assert set(grad) == set(m.get_params())
        scale = _check_numpy(m, x, y, ll, grad)
        _check_single(m, ds, ll, grad, scale)


def test_batch_of_dimensions_2_4_5(ctx):
    """One launch on Point<8> for problems of 2, 4 and 5 dimensions: the zero-padding of every problem's points up to
    the batch's largest dimension.  n = 130: full and partial tiles of both kinds.  cond(K) = 8.3e3, 3.7e3, 8.5e2 (numpy)."""
    problems = []
    for dim in (2, 4, 5):
        model = ab.gp_from_covariance(ab.SquaredExponential(1.5, 1.2) + ab.IndependentNoise(0.1), context=ctx)
        problems.append((model, *_padded_data(dim)))
    datasets = [ab.RegressionDataset(x, y) for _, x, y in problems]
    out = ab.log_likelihood_gradient_batch([m for m, _, _ in problems], datasets)
    assert len(out) == len(problems)
    for (m, x, y), ds, (ll, grad) in zip(problems, datasets, out):
        assert set(grad) == set(m.get_params())
        scale = _check_numpy(m, x, y, ll, grad)
        _check_single(m, ds, ll, grad, scale)


def _bits(results):
    return [(np.float64(ll).tobytes(), tuple(sorted((k, np.float64(v).tobytes()) for k, v in g.items()))) for ll, g in results]


def test_deterministic_and_permutation_invariant(ctx):
    n = 300
    problems = _heterogeneous(ctx, n)
    models = [m for m, _, _ in problems]
    datasets = [ab.RegressionDataset(x, y) for _, x, y in problems]
    first = _bits(ab.log_likelihood_gradient_batch(models, datasets))
    assert _bits(ab.log_likelihood_gradient_batch(models, datasets)) == first
    rev = _bits(ab.log_likelihood_gradient_batch(models[::-1], datasets[::-1]))
    assert rev[::-1] == first


def test_result_does_not_depend_on_the_neighbours(ctx):
    """problem 0 in two batches of the same count whose other problems differ (same trees and dimension)"""
    x, y = synthetic_3d(512, 3)
    model = _config3(ctx)
    ds = ab.RegressionDataset(x, y)
    mine = {"sigma_squared_exponential": 1.3}
    a = model.log_likelihood_gradients(ds, [mine] + _sets(model, 8, 1)[1:])
    b = model.log_likelihood_gradients(ds, [mine] + _sets(model, 8, 2)[1:])
    assert np.float64(a[0][0]).tobytes() == np.float64(b[0][0]).tobytes()
    assert all(np.float64(a[1][0][k]).tobytes() == np.float64(b[1][0][k]).tobytes() for k in a[1][0])


# ---- the C-ABI directly -------------------------------------------------------------------------------------------
class _Raw:
    """the arguments of one agp_nll_gradient_batch call, built from (model, x, y) problems, with every array kept alive"""

    def __init__(self, ctx, problems):
        self.ctx = ctx
        self.models = [m for m, _, _ in problems]
        self.probs = [abgp._gradient_problem(m, ab.RegressionDataset(x, y)) for m, x, y in problems]
        self.count = len(problems)
        self.n = self.probs[0].fs.n
        self.structs = [p.fs.as_struct() for p in self.probs]
        self.Y = np.asfortranarray(np.stack([p.y for p in self.probs], axis=1))
        self.ldg = max(1, max(len(p.slots) for p in self.probs))
        self.n_slots = (C.c_int * self.count)(*[len(p.slots) for p in self.probs])
        self.tables = (C.c_void_p * self.count)(*[C.addressof(p.table) for p in self.probs])
        self.tang = (C.c_void_p * self.count)(*[None if p.tangents is None else p.tangents.ctypes.data for p in self.probs])
        self.ldt = self.n
        self.y_ptr = _p(self.Y)
        self.ldy = self.n

    def call(self, **over):
        ctx = self.ctx
        count = over.get("count", self.count)
        nll = np.full(self.count, 7.0)
        grad = np.full((self.count, self.ldg), 7.0)
        info = np.full((self.count, self.n), 7.0)
        status = (C.c_int * self.count)(*([-5] * self.count))
        handles = [ctx.private_kernel(m.covariance_function_) for m in self.models]
        try:
            kernels = (C.c_void_p * self.count)(*handles)
            fptrs = (C.c_void_p * self.count)(*[C.addressof(s) for s in self.structs])
            rc = ctx._lib.agp_nll_gradient_batch(ctx._h, count, kernels, fptrs, over.get("y", self.y_ptr), over.get("ldy", self.ldy),
                                                 None, 0, over.get("n_slots", self.n_slots), over.get("slots", self.tables),
                                                 over.get("tangents", self.tang), over.get("ldt", self.ldt), _p(nll), _p(grad),
                                                 over.get("ldg", self.ldg), _p(info), self.n, status)
        finally:
            for h in handles:
                ctx._lib.agp_kernel_destroy(h)
        return rc, nll, grad, info, list(status)


def test_failed_problems_are_reported_and_isolated(ctx):
    n = 300
    rng = np.random.default_rng(4)
    problems = []
    for b in range(6):
        x = rng.uniform(0., 10., (n, 3))
        problems.append((_config3(ctx), x, np.sin(x).sum(axis=1)))
    xs = problems[1][1].copy()
    xs[5] = xs[0]  # no noise + a duplicated point: singular
    problems[1] = (ab.gp_from_covariance(ab.SquaredExponential(1., 1.), context=ctx), xs, problems[1][2])
    xn = problems[4][1].copy()
    xn[17, 1] = np.nan
    problems[4] = (problems[4][0], xn, problems[4][2])
    raw = _Raw(ctx, problems)
    rc, nll, grad, info, status = raw.call()
    assert rc == capi.AGP_OK
    assert status[1] == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and status[4] == capi.AGP_ERR_NAN_INPUT
    for b in (1, 4):
        assert np.isnan(nll[b]) and np.isnan(grad[b, :raw.n_slots[b]]).all()
        assert (info[b] == 7.0).all()  # left untouched
    for b in (0, 2, 3, 5):
        assert status[b] == capi.AGP_OK
        m, x, y = problems[b]
        ds = ab.RegressionDataset(x, y)
        ll1, g1 = m.log_likelihood_gradient(ds)
        assert abs(-nll[b] - ll1) <= 1e-10 * max(1., abs(ll1))
        grad_b = m._log_likelihood_gradient_dict(raw.probs[b].slots, grad[b, :raw.n_slots[b]], info[b], raw.probs[b].fs)
        scale = reference_gradient(m, x, y)[1]
        for k in g1:
            assert abs(grad_b[k] - g1[k]) <= 1e-9 * scale[k], k
    # the Python layers give NaN, not an exception
    out = ab.log_likelihood_gradient_batch([m for m, _, _ in problems], [ab.RegressionDataset(x, y) for _, x, y in problems])
    assert np.isnan(out[1][0]) and all(np.isnan(v) for v in out[4][1].values())
    assert not np.isnan(out[0][0])


def test_not_positive_definite_set_gives_nan(ctx):
    rng = np.random.default_rng(8)
    x = rng.uniform(0., 10., (200, 3))
    x[1] = x[0]  # without noise: K_00 = K_01 = K_11 = 1 exactly, the second pivot is 0
    model = _config3(ctx)
    lls, grads = model.log_likelihood_gradients(ab.RegressionDataset(x, np.sin(x).sum(axis=1)),
                                                [{}, {"sigma_independent_noise": 0.0}, {"sigma_squared_exponential": 1.2}])
    assert np.isnan(lls[1]) and all(np.isnan(v) for v in grads[1].values())
    assert not np.isnan(lls[0]) and not np.isnan(lls[2])


def test_argument_errors_write_nothing(ctx):
    n = 100
    rng = np.random.default_rng(2)
    x = rng.uniform(0., 10., (n, 3))
    _, elev = _elevation_model(ctx)
    problems = [(_config3(ctx), x, np.sin(x).sum(axis=1)), (elev, x, np.cos(x).sum(axis=1))]
    raw = _Raw(ctx, problems)
    rc, nll, grad, info, status = raw.call()
    assert rc == capi.AGP_OK and status == [0, 0]

    def rejected(**over):
        rc, nll, grad, info, status = raw.call(**over)
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT, over
        assert (nll == 7.0).all() and (grad == 7.0).all() and (info == 7.0).all() and status == [-5, -5], over

    rejected(count=0)
    rejected(count=-1)
    rejected(ldy=n - 1)
    rejected(ldg=raw.ldg - 1)
    rejected(ldt=n - 1)
    rejected(tangents=None)
    rejected(tangents=(C.c_void_p * 2)(raw.tang[0], None))
    rejected(n_slots=(C.c_int * 2)(raw.n_slots[0], capi.MAX_GRADIENT_SLOTS + 1))
    rejected(n_slots=(C.c_int * 2)(-1, raw.n_slots[1]))
    bad = (capi.GradientSlot * 1)(capi.GradientSlot(2, 0))  # the sum node of SE + noise
    rejected(slots=(C.c_void_p * 2)(C.addressof(bad), raw.tables[1]), n_slots=(C.c_int * 2)(1, raw.n_slots[1]))
    rejected(slots=(C.c_void_p * 2)(None, raw.tables[1]))
    # n mismatch and mixed locations
    raw2 = _Raw(ctx, problems)
    raw2.structs[1].n = n - 1
    rc, nll, grad, info, status = raw2.call()
    assert rc == capi.AGP_ERR_INVALID_ARGUMENT and (nll == 7.0).all() and status == [-5, -5]
    raw3 = _Raw(ctx, problems)
    raw3.structs[1].location = capi.DEVICE
    rc, nll, grad, info, status = raw3.call()
    assert rc == capi.AGP_ERR_INVALID_ARGUMENT and (grad == 7.0).all() and status == [-5, -5]


def test_device_resident_inputs_give_the_same_bits(ctx):
    n = 300
    rng = np.random.default_rng(12)
    x = rng.uniform(0., 10., (n, 3))
    _, elev = _elevation_model(ctx)
    problems = [(elev, x, np.sin(x).sum(axis=1)), (_copy(elev, {"elevation_scaling_center": 6.0}), x, np.cos(x).sum(axis=1)),
                (_config3(ctx), x, np.sin(x[:, 0]))]
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
    yd = dev(raw.Y)
    tang = []
    for p in raw.probs:
        if p.tangents is None:
            tang.append(None)
        else:
            td = dev(p.tangents)
            keep.append(td)
            tang.append(td.ptr)
    dev = raw.call(y=C.c_void_p(yd.ptr), tangents=(C.c_void_p * 3)(*tang))
    assert dev[0] == capi.AGP_OK and dev[4] == [0, 0, 0]
    for h, d in zip(host[1:4], dev[1:4]):
        assert h.tobytes() == d.tobytes()
    for d in keep + [yd]:
        d.free()


# ---- the batched R^T R kernel alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128, 300, 512])
@pytest.mark.parametrize("count", [1, 5, 64])
def test_batched_rtr_kernel_matches_numpy(ctx, count, n):
    dbg = capi.load_debug()
    dbg.agp_debug_rtr_lower_batched.restype = C.c_int
    dbg.agp_debug_rtr_lower_batched.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                C.POINTER(C.c_double)]
    rng = np.random.default_rng(count * 1000 + n)
    ld = n + 8
    Rd = np.zeros((count, n, ld))  # slab b: column-major ld x n = row-major n x ld
    Rs = []
    for b in range(count):
        R = np.tril(rng.uniform(-1., 1., (n, n))) / np.sqrt(n)
        R[np.diag_indices(n)] = 1. + rng.uniform(0., 1., n)
        Rs.append(R)
        Rd[b, :, :n] = R.T
    Cd = np.zeros_like(Rd)
    ms = C.c_double()
    assert dbg.agp_debug_rtr_lower_batched(ctx._h, _p(Rd), n, ld, count, _p(Cd), C.byref(ms)) == 0
    low = np.tril_indices(n)
    for b in range(count):
        want = Rs[b].T @ Rs[b]
        got = Cd[b, :, :n].T
        assert np.abs(got[low] - want[low]).max() <= 1e-13 * np.abs(want).max(), b
    if count == 1:
        dbg.agp_debug_rtr_lower.restype = C.c_int
        dbg.agp_debug_rtr_lower.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_double)]
        C1 = np.zeros_like(Rd)
        assert dbg.agp_debug_rtr_lower(ctx._h, _p(Rd), n, ld, _p(C1), C.byref(ms)) == 0
        got, single = Cd[0, :, :n].T, C1[0, :, :n].T
        assert got[low].tobytes() == single[low].tobytes()


def test_cpp_gradients_match_python(ctx):
    """examples/gradient_batch_check (GaussianProcessRegression::log_likelihood_gradients) against log_likelihood_gradients"""
    import os
    import subprocess
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "gradient_batch_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y = data[:, 1:4], data[:, 4]
    cov, _ = _elevation_model(ctx)
    model = ab.gp_from_covariance_and_mean(cov, _FirstCoordinateMean(0.2, -0.4), context=ctx)
    sets = [{}, {"elevation_scaling_center": 5.0}, {"sigma_matern_52": 1.3, "slope": 0.5},
            {"elevation_scaling_factor": 0.5, "sigma_independent_noise": 0.2, "offset": 0.1}]
    lls, grads = model.log_likelihood_gradients(ab.RegressionDataset(x, y), sets)
    cpp_ll = {int(b): float(v) for b, v in rows["loglik"]}
    assert sorted(cpp_ll) == list(range(len(sets)))
    for b in range(len(sets)):
        assert abs(cpp_ll[b] - lls[b]) <= 1e-10 * abs(lls[b])
        cpp = {k[len("grad_"):]: float(v) for k, vs in rows.items() if k.startswith("grad_") for bb, v in vs if int(bb) == b}
        assert set(cpp) == set(grads[b])
        big = max(abs(g) for g in grads[b].values())
        for name, g in grads[b].items():
            assert abs(cpp[name] - g) <= 1e-10 * max(abs(g), 1e-3 * big), (b, name)


def test_repeated_calls_return_device_memory(ctx):
    import gc
    import torch
    n = 300
    problems = _heterogeneous(ctx, n)
    models = [m for m, _, _ in problems]
    datasets = [ab.RegressionDataset(x, y) for _, x, y in problems]
    x, y = synthetic_3d(512, 9)
    model = _config3(ctx)
    ds = ab.RegressionDataset(x, y)

    def cycle():
        ab.log_likelihood_gradient_batch(models, datasets)
        model.log_likelihood_gradients(ds, _sets(model, 16, 4))

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
