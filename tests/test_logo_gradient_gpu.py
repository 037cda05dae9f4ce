"""GPU tests of the leave-one-group-out likelihood metric and its exact gradient: agp_logo_nll_gradient,
GaussianProcessRegression.leave_one_group_out_likelihood_gradient and LeaveOneGroupOutLikelihood.

Reference: numpy, independent of the library.  K = orc.gram(measurement features) + diag(s), and from it the value,
S = C B C, u and alpha by the closed form that tests/test_logo_gradient_host.py checks against brute-force refits
(logo_closed_form).  dK / dtheta is a central difference of orc.gram at theta +- h, h = 1e-5 max(1, |theta|); mean
terms -u^T dmu / dtheta with central differences of orc.mean_vector.

Tolerances, those of tests/test_loo_gradient_gpu.py (whose docstring derives them): the value to 1e-10 relative,
|g - g_ref| <= 1e-7 s_p with s_p = sum |S o dK| + sum |sym(u alpha^T) o dK|, the sum of the magnitudes of the terms the
gradient adds up.

Shapes: the smallest that cross every edge.  n = 300 is three 128-tiles of the products with a partial last one and
five contraction tiles; its ragged grouping has a group wider than one 128 panel of the block factorisation (130), odd
sizes, sizes on both sides of every power of two up to 128 (several size classes, each padded) and 26 singletons;
n = 256 in 64 groups of 4 has no padding anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from oracle import oracle_py as orc
from test_logo_gradient_host import LOG_2PI, logo_brute_force, logo_closed_form
from test_nll_gradient_gpu import LEAVES, _data, _elevation_model, _FirstCoordinateMean, perturbed

pytestmark = pytest.mark.gpu

RAGGED_SIZES = [130, 65, 33, 17, 16, 7, 3, 2, 1] + [1] * 26


def ragged_groups(n=300, seed=41, sizes=RAGGED_SIZES):
    """groups of the given sizes from a random permutation: indices unsorted inside the groups"""
    assert sum(sizes) == n
    perm = np.random.default_rng(seed).permutation(n)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return {g: perm[edges[g]:edges[g + 1]].tolist() for g in range(len(sizes))}


def reference(model, x, y, s, groups, threads=16, brute=False):
    """({name: d LOGO / d name}, {name: s_p}, value[, brute-force value], [B_g]) in numpy from the oracle's Gram matrices"""
    cov, mean = model.covariance_function_, model.mean_function_
    sv = np.zeros(len(y)) if s is None else s
    K = orc.gram(cov, x, x_meas=True, threads=threads) + np.diag(sv)
    r = np.asarray(y, dtype=np.float64) - orc.mean_vector(mean, cov, x)
    value, W, u, alpha, blocks = logo_closed_form(K, r, sv, groups)
    sym = 0.5 * (np.outer(u, alpha) + np.outer(alpha, u))
    S = W + sym
    grads, scales = {}, {}
    cov_names = cov.get_params()
    for name, val in model.get_params().items():
        h = 1e-5 * max(1., abs(val))
        (cov_up, mean_up), (cov_down, mean_down) = perturbed(model, name, val + h), perturbed(model, name, val - h)
        if name in cov_names:
            dK = (orc.gram(cov_up, x, x_meas=True, threads=threads) - orc.gram(cov_down, x, x_meas=True, threads=threads)) / (2 * h)
            grads[name] = np.sum(S * dK) - np.sum(sym * dK)
            scales[name] = np.sum(np.abs(S * dK)) + np.sum(np.abs(sym * dK))
        else:
            dmu = (orc.mean_vector(mean_up, cov, x) - orc.mean_vector(mean_down, cov, x)) / (2 * h)
            grads[name] = -u @ dmu
            scales[name] = np.abs(u) @ np.abs(dmu)
    bf = logo_brute_force(K, r, sv, groups) if brute else None
    return grads, scales, value, bf, blocks


def _dataset(x, y, s):
    return ab.RegressionDataset(x, ab.MarginalDistribution(y, s))


def check(model, x, y, s, indexer, brute=False):
    ds = _dataset(x, y, s)
    logo, grad = model.leave_one_group_out_likelihood_gradient(ds, indexer)
    assert set(grad) == set(model.get_params())
    want, scale, value, bf, blocks = reference(model, x, y, s, list(indexer.values()), brute=brute)
    print("value", logo, value, bf)
    assert abs(logo - value) <= 1e-10 * abs(value), (logo, value)
    if brute:
        assert abs(logo - bf) <= 1e-10 * abs(bf), (logo, bf)
    for name in want:
        print(name, grad[name], want[name], abs(grad[name] - want[name]) / scale[name])
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    # the value-only call builds the blocks from gathered columns of R, the full call from C = R^T R
    alone = ab.LeaveOneGroupOutLikelihood(indexer)(ds, model)
    assert abs(alone - value) <= 1e-10 * abs(value), (alone, value)
    return logo, grad, blocks


def _variance(n, seed):
    return np.random.default_rng(seed).uniform(0.005, 0.05, n)


def _m52(ctx):
    return ab.gp_from_covariance(ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)


@pytest.mark.parametrize("with_variance", [False, True])
def test_ragged_groups_300(ctx, with_variance):
    x, y = _data(300, 3, 331)
    s = _variance(300, 300) if with_variance else None
    check(_m52(ctx), x, y, s, ragged_groups(), brute=True)


@pytest.mark.parametrize("label,make,dim", LEAVES)
def test_groups_of_four_256_every_leaf(ctx, label, make, dim):
    x, y = _data(256, dim, 267)
    indexer = {g: list(range(4 * g, 4 * g + 4)) for g in range(64)}
    check(ab.gp_from_covariance(make(), context=ctx), x, y, _variance(256, 5), indexer)


def test_groups_of_four_256_scaling_term_and_linear_mean(ctx):
    x, y = _data(256, 3, 259)
    y = y + 0.3 * x[:, 0]
    _, model = _elevation_model(ctx)
    model.set_param_values({"slope": 0.2, "offset": -0.4})
    indexer = {g: list(range(4 * g, 4 * g + 4)) for g in range(64)}
    _, grad, _ = check(model, x, y, _variance(256, 6), indexer)
    assert {"elevation_scaling_center", "elevation_scaling_factor", "slope", "offset"} <= set(grad)


@pytest.mark.parametrize("with_variance", [False, True])
def test_one_group_is_the_likelihood_of_everything(ctx, with_variance):
    n = 200
    x, y = _data(n, 3, 201)
    s = _variance(n, 7) if with_variance else None
    model = _m52(ctx)
    indexer = {0: np.random.default_rng(3).permutation(n).tolist()}
    logo, _, _ = check(model, x, y, s, indexer)
    sv = np.zeros(n) if s is None else s
    M = orc.gram(model.covariance_function_, x, x_meas=True) + 2. * np.diag(sv)  # K + diag(s), K = cov + diag(s)
    want = 0.5 * (np.linalg.slogdet(M)[1] + y @ np.linalg.solve(M, y) + n * LOG_2PI)
    assert abs(logo - want) <= 1e-10 * abs(want), (logo, want)


@pytest.mark.parametrize("with_variance", [False, True])
def test_singletons_300_equal_leave_one_out(ctx, with_variance):
    n = 300
    x, y = _data(n, 3, 311)
    s = _variance(n, 8) if with_variance else None
    _, model = _elevation_model(ctx)
    ds = _dataset(x, y, s)
    logo, grad = model.leave_one_group_out_likelihood_gradient(ds, ab.LeaveOneOutGrouper())
    loo, loo_grad = model.leave_one_out_likelihood_gradient(ds)
    _, scale, _, _, _ = reference(model, x, y, s, [[i] for i in range(n)])
    assert abs(logo - loo) <= 1e-10 * abs(loo), (logo, loo)
    for name in loo_grad:
        assert abs(grad[name] - loo_grad[name]) <= 1e-7 * scale[name], (name, grad[name], loo_grad[name])
    alone = ab.LeaveOneGroupOutLikelihood(ab.LeaveOneOutGrouper())(ds, model)
    assert abs(alone - ab.LeaveOneOutLikelihood()(ds, model)) <= 1e-10 * abs(loo)


def test_indefinite_blocks_300(ctx):
    """large target variances and residuals: a block of the weight has a negative eigenvalue,
    checked in numpy before the library is called"""
    n = 300
    rng = np.random.default_rng(23)
    x = rng.uniform(0., 5., (n, 2))
    s = rng.uniform(0.01, 2., n)
    y = 5. * np.sin(x).sum(axis=1) + 5. * np.sqrt(s) * rng.standard_normal(n)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.3, 0.9) + ab.IndependentNoise(0.2), context=ctx)
    indexer = ragged_groups()
    K = orc.gram(model.covariance_function_, x, x_meas=True) + np.diag(s)
    blocks = logo_closed_form(K, y, s, list(indexer.values()))[4]
    lowest = min(np.linalg.eigvalsh(b).min() for b in blocks)
    print("lowest eigenvalue of a block", lowest)
    assert lowest < -0.1
    check(model, x, y, s, indexer, brute=True)


def test_partial_cover_and_empty_group(ctx):
    n = 300
    x, y = _data(n, 3, 17)
    s = _variance(n, 18)
    perm = np.random.default_rng(19).permutation(n)
    indexer = {"a": perm[:40].tolist(), "empty": [], "b": perm[40:45].tolist(), "c": perm[45:46].tolist(),
               "d": perm[46:180].tolist()}  # 120 points are in no group
    check(_m52(ctx), x, y, s, indexer, brute=True)
    assert ab.LeaveOneGroupOutLikelihood({})(_dataset(x, y, s), _m52(ctx)) == 0.


def test_size_class_split_into_two_chunks(ctx):
    """60 groups of 2 and 60 of 3 are one size class, but padded to 3 they are 360 columns, more than the n = 300 a chunk
    may hold: the class advances as two chunks (100 groups, then 20), whose terms and blocks must land where one chunk's
    would"""
    n = 300
    x, y = _data(n, 3, 77)
    perm = np.random.default_rng(78).permutation(n)
    indexer = {g: perm[3 * g:3 * g + 3].tolist() for g in range(60)}
    indexer.update({60 + g: perm[180 + 2 * g:182 + 2 * g].tolist() for g in range(60)})
    check(_m52(ctx), x, y, _variance(n, 79), indexer, brute=True)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class _Raw:
    """one problem of n = 60 points for direct calls of the entry"""

    def __init__(self, ctx, n=60):
        self.ctx = ctx
        self.x, self.y = _data(n, 2, 6)
        self.s = _variance(n, 2)
        self.cov = ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1)  # nodes: 0 SE, 1 noise, 2 sum
        self.fs = self.cov.features(self.x)
        self.struct = self.fs.as_struct()
        self.n = n

    def call(self, offsets, indices, slots=((0, 0), (0, 1), (1, 0)), struct=None, y=None, s=None):
        offsets, indices = np.asarray(offsets, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        table = (capi.GradientSlot * max(1, len(slots)))(*[capi.GradientSlot(a, b) for a, b in slots])
        value = C.c_double(-7.)
        grad, u = np.full(max(1, len(slots)), -7.), np.full(self.n, -7.)
        st = self.ctx._lib.agp_logo_nll_gradient(self.ctx._h, self.ctx.kernel(self.cov), C.byref(struct or self.struct),
                                                 y or _p(self.y), s or _p(self.s), len(offsets) - 1, _p(offsets), _p(indices),
                                                 len(slots), table, None, 0, C.byref(value), _p(grad), _p(u))
        return st, value.value, grad, u


def test_malformed_calls_write_nothing(ctx):
    raw = _Raw(ctx)
    n = raw.n
    good = (np.array([0, 3, 3, 10]), np.array([5, 1, 9, 20, 21, 22, 23, 24, 25, 59]))
    st, value, grad, u = raw.call(*good)
    assert st == capi.AGP_OK and value != -7. and np.all(grad[:3] != -7.) and np.all(u != -7.)

    def refused(offsets, indices, slots=((0, 0), (0, 1), (1, 0))):
        st, value, grad, u = raw.call(offsets, indices, slots)
        assert st == capi.AGP_ERR_INVALID_ARGUMENT
        assert value == -7. and np.all(grad == -7.) and np.all(u == -7.)

    refused([0, 3, 3, 10], [5, 1, 5, 20, 21, 22, 23, 24, 25, 59])    # an index twice in one group
    refused([0, 3, 3, 10], [5, 1, 9, 20, 21, 22, 23, 24, 9, 59])     # an index in two groups
    refused([0, 3, 3, 10], [5, 1, 9, 20, 21, 22, 23, 24, 25, n])     # out of range
    refused([0, 3, 3, 10], [5, 1, 9, 20, 21, -1, 23, 24, 25, 59])
    refused([1, 3, 3, 10], good[1])                                  # offsets[0] != 0
    refused([0, 3, 2, 10], good[1])                                  # offsets not monotone
    refused(*good, slots=((2, 0),))                                  # the sum node
    refused(*good, slots=((0, 2),))                                  # a radial leaf has two parameters
    refused(*good, slots=((0, 0),) * (capi.MAX_GRADIENT_SLOTS + 1))


def test_deterministic(ctx):
    n = 300
    x, y = _data(n, 3, 2)
    _, model = _elevation_model(ctx)
    ds = _dataset(x, y, _variance(n, 3))
    indexer = ragged_groups(seed=4)
    v1, g1 = model.leave_one_group_out_likelihood_gradient(ds, indexer)
    v2, g2 = model.leave_one_group_out_likelihood_gradient(ds, indexer)
    assert v1 == v2
    assert all(g1[k] == g2[k] for k in g1)
    metric = ab.LeaveOneGroupOutLikelihood(indexer)
    assert metric(ds, model) == metric(ds, model)


def test_value_only_path_forms_no_inverse(ctx):
    """with profiling on: the value-only call reports 0 for R^T R (6), the product (9) and the contraction (7)"""
    n = 300
    x, y = _data(n, 3, 12)
    model = _m52(ctx)
    ds = _dataset(x, y, _variance(n, 13))
    indexer = ragged_groups(seed=5)
    ctx.set_profiling(True)
    try:
        full, _ = model.leave_one_group_out_likelihood_gradient(ds, indexer)
        assert ctx.stage_ms(6) > 0. and ctx.stage_ms(9) > 0. and ctx.stage_ms(7) > 0. and ctx.stage_ms(8) > 0.
        alone = ab.LeaveOneGroupOutLikelihood(indexer)(ds, model)
        assert ctx.stage_ms(6) == 0. and ctx.stage_ms(9) == 0. and ctx.stage_ms(7) == 0.
        assert ctx.stage_ms(8) > 0. and ctx.stage_ms(2) > 0.
    finally:
        ctx.set_profiling(False)
    assert abs(alone - full) <= 1e-12 * abs(full), (alone, full)


def test_callable_grouper_equals_the_entry(ctx):
    n = 300
    x, y = _data(n, 3, 21)
    s = _variance(n, 22)
    model = _m52(ctx)
    ds = _dataset(x, y, s)

    def station(feature):
        return int(feature[0])

    indexer = ab.group_indexer(x, station)
    assert len(indexer) == 10
    value = ab.LeaveOneGroupOutLikelihood(station)(ds, model)
    full, grad = model.leave_one_group_out_likelihood_gradient(ds, station)
    groups = list(indexer.values())
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    indices = np.concatenate(groups).astype(np.int64)
    cov = model.covariance_function_
    fs = cov.features(x)
    st = fs.as_struct()
    out = C.c_double()
    assert ctx._lib.agp_logo_nll_gradient(ctx._h, ctx.kernel(cov), C.byref(st), _p(y), _p(s), len(groups), _p(offsets), _p(indices),
                                          0, None, None, 0, C.byref(out), None, None) == capi.AGP_OK
    assert value == out.value
    assert abs(full - value) <= 1e-12 * abs(value)
    assert set(grad) == set(model.get_params())


def test_device_resident_inputs_equal_host_inputs(ctx):
    raw = _Raw(ctx, n=300)
    indexer = ragged_groups(seed=6)
    groups = list(indexer.values())
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    indices = np.concatenate(groups)
    host = raw.call(offsets, indices)
    assert host[0] == capi.AGP_OK
    keep = [ctx.to_device(np.ravel(raw.fs.coords, order="K")), ctx.to_device(raw.y), ctx.to_device(raw.s)]
    struct = raw.cov.features(raw.x).as_struct()
    struct.coords = keep[0].ptr
    assert raw.fs.scales is None
    struct.location = capi.DEVICE
    dev = raw.call(offsets, indices, struct=struct, y=C.c_void_p(keep[1].ptr), s=C.c_void_p(keep[2].ptr))
    assert dev[0] == capi.AGP_OK
    assert host[1] == dev[1] and host[2].tobytes() == dev[2].tobytes() and host[3].tobytes() == dev[3].tobytes()
    for d in keep:
        d.free()


def test_errors(ctx):
    x, _ = _data(20, 2, 4)
    xd = np.concatenate([x[:10], x[:10]])
    indexer = {0: list(range(10)), 1: list(range(10, 20))}
    bad = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0), context=ctx)
    with pytest.raises(ab.NotPositiveDefiniteError):
        bad.leave_one_group_out_likelihood_gradient(ab.RegressionDataset(xd, np.zeros(20)), indexer)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    with pytest.raises(NotImplementedError):
        model.leave_one_group_out_likelihood_gradient(ab.RegressionDataset(lc, np.zeros(2)), {0: [0, 1]})
    with pytest.raises(NotImplementedError):
        ab.LeaveOneGroupOutLikelihood({0: [0, 1]})(ab.RegressionDataset(lc, np.zeros(2)), model)
    mixed = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    mixed.precision = "mixed"
    with pytest.raises(ValueError):
        mixed.leave_one_group_out_likelihood_gradient(ab.RegressionDataset(x, np.zeros(20)), indexer)
    with pytest.raises(ValueError):
        ab.LeaveOneGroupOutLikelihood(indexer)(ab.RegressionDataset(x, np.zeros(20)), mixed)


def test_cpp_logo_gradient_matches_python(ctx):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "logo_gradient_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y, s = data[:, 1:4], data[:, 4], data[:, 5]
    cov, _ = _elevation_model(ctx)
    model = ab.gp_from_covariance_and_mean(cov, _FirstCoordinateMean(0.2, -0.4), context=ctx)
    ds = _dataset(x, y, s)

    def station(feature):
        return str(int(feature[0]))

    logo, grad = model.leave_one_group_out_likelihood_gradient(ds, station)
    cpp = {k[len("grad_"):]: float(v[0][0]) for k, v in rows.items() if k.startswith("grad_")}
    assert set(cpp) == set(grad)
    assert abs(float(rows["logo_nll"][0][0]) - logo) <= 1e-10 * abs(logo)
    assert abs(float(rows["logo_nll_metric"][0][0]) - ab.LeaveOneGroupOutLikelihood(station)(ds, model)) <= 1e-10 * abs(logo)
    for name in grad:
        assert abs(cpp[name] - grad[name]) <= 1e-10 * max(abs(grad[name]), 1e-3 * max(abs(g) for g in grad.values())), name
