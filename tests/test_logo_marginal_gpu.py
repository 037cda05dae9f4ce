"""GPU tests of the leave-one-group-out likelihood metric with the MARGINAL predict type, its exact gradient and the
per-group terms: agp_logo_nll_gradient_typed, GaussianProcessRegression.leave_one_group_out_likelihood_gradient(...,
predict_type="marginal"), LeaveOneGroupOutLikelihood(grouper, "marginal") and its group_scores.

Reference: numpy, independent of the library.  K = orc.gram(measurement features) + diag(s), and from it the value, the
per-group terms, S = C B C, u and alpha by the closed form that tests/test_logo_marginal_host.py checks against
brute-force refits (logo_marginal_closed_form).  dK / dtheta and the scales s_p exactly as reference() of
tests/test_logo_gradient_gpu.py builds them.

Tolerances, those of tests/test_logo_gradient_gpu.py: the value to 1e-10 relative, |g - g_ref| <= 1e-7 s_p.  Shapes:
that file's smallest-edge shapes (n = 300 ragged with a group of 130 wider than one 128 panel, so that the two-operand
block product crosses a tile edge, and several padded size classes; n = 256 in 64 groups of 4 without padding; one
group of everything; singletons; a partial cover with an empty group; a size class cut into two chunks)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from oracle import oracle_py as orc
from test_logo_gradient_gpu import _dataset, _m52, _p, _variance, ragged_groups
from test_logo_gradient_host import LOG_2PI, logo_closed_form
from test_logo_marginal_host import logo_marginal_brute_force, logo_marginal_closed_form
from test_nll_gradient_gpu import LEAVES, _data, _elevation_model, _FirstCoordinateMean, perturbed

pytestmark = pytest.mark.gpu


def reference(model, x, y, s, groups, threads=16, brute=False):
    """({name: d LOGO / d name}, {name: s_p}, value[, brute-force value], [B_g], [NLL_g]) in numpy from the oracle's Gram
    matrices, Marginal predict type"""
    cov, mean = model.covariance_function_, model.mean_function_
    sv = np.zeros(len(y)) if s is None else s
    K = orc.gram(cov, x, x_meas=True, threads=threads) + np.diag(sv)
    r = np.asarray(y, dtype=np.float64) - orc.mean_vector(mean, cov, x)
    value, W, u, alpha, blocks, terms = logo_marginal_closed_form(K, r, sv, groups)
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
    bf = logo_marginal_brute_force(K, r, sv, groups) if brute else None
    return grads, scales, value, bf, blocks, terms


def check(model, x, y, s, indexer, brute=False):
    ds = _dataset(x, y, s)
    logo, grad = model.leave_one_group_out_likelihood_gradient(ds, indexer, predict_type="marginal")
    assert set(grad) == set(model.get_params())
    want, scale, value, bf, blocks, terms = reference(model, x, y, s, list(indexer.values()), brute=brute)
    print("value", logo, value, bf)
    assert abs(logo - value) <= 1e-10 * abs(value), (logo, value)
    if brute:
        assert abs(logo - bf) <= 1e-10 * abs(bf), (logo, bf)
    for name in want:
        print(name, grad[name], want[name], abs(grad[name] - want[name]) / scale[name])
        assert abs(grad[name] - want[name]) <= 1e-7 * scale[name], (name, grad[name], want[name], scale[name])
    # the value-only call builds the blocks from gathered columns of R, the full call from C = R^T R
    metric = ab.LeaveOneGroupOutLikelihood(indexer, "marginal")
    alone = metric(ds, model)
    print("value only", alone)
    assert abs(alone - value) <= 1e-10 * abs(value), (alone, value)
    assert abs(alone - logo) <= 1e-10 * abs(logo), (alone, logo)
    # the per-group terms of the same call, in the caller's order
    scores = metric.group_scores(ds, model)
    assert list(scores) == list(indexer)
    for key, t in zip(indexer, terms):
        assert abs(scores[key] - t) <= 1e-10 * max(1., abs(t)), (key, scores[key], t)
    return logo, grad, blocks


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
def test_one_group_scores_every_point_against_its_prior_variance(ctx, with_variance):
    """one group of everything: Sigma = K and d = y, so v_i = k_ii + 2 s_i with k the covariance function's own
    diagonal - a number the Joint type (the likelihood of everything) cannot produce"""
    n = 200
    x, y = _data(n, 3, 201)
    s = _variance(n, 7) if with_variance else None
    model = _m52(ctx)
    indexer = {0: np.random.default_rng(3).permutation(n).tolist()}
    logo, _, _ = check(model, x, y, s, indexer)
    sv = np.zeros(n) if s is None else s
    v = np.diag(orc.gram(model.covariance_function_, x, x_meas=True)) + 2. * sv
    want = 0.5 * np.sum(np.log(v) + y * y / v + LOG_2PI)
    assert abs(logo - want) <= 1e-10 * abs(want), (logo, want)
    joint = ab.LeaveOneGroupOutLikelihood(indexer)(_dataset(x, y, s), model)
    assert abs(joint - want) > 1e-3 * abs(want)


@pytest.mark.parametrize("with_variance", [False, True])
def test_singletons_300_equal_leave_one_out_and_the_joint_type(ctx, with_variance):
    n = 300
    x, y = _data(n, 3, 311)
    s = _variance(n, 8) if with_variance else None
    _, model = _elevation_model(ctx)
    ds = _dataset(x, y, s)
    grouper = ab.LeaveOneOutGrouper()
    logo, grad = model.leave_one_group_out_likelihood_gradient(ds, grouper, predict_type="marginal")
    loo, loo_grad = model.leave_one_out_likelihood_gradient(ds)
    joint, joint_grad = model.leave_one_group_out_likelihood_gradient(ds, grouper)
    scale = reference(model, x, y, s, [[i] for i in range(n)])[1]
    assert abs(logo - loo) <= 1e-10 * abs(loo), (logo, loo)
    assert abs(logo - joint) <= 1e-10 * abs(joint), (logo, joint)
    for name in loo_grad:
        assert abs(grad[name] - loo_grad[name]) <= 1e-7 * scale[name], (name, grad[name], loo_grad[name])
        assert abs(grad[name] - joint_grad[name]) <= 1e-7 * scale[name], (name, grad[name], joint_grad[name])
    alone = ab.LeaveOneGroupOutLikelihood(grouper, "marginal")(ds, model)
    assert abs(alone - ab.LeaveOneOutLikelihood()(ds, model)) <= 1e-10 * abs(loo)


def test_indefinite_blocks_300(ctx):
    """large target variances and residuals: w_i < 0 for many points and a block of the weight has a negative
    eigenvalue, checked in numpy before the library is called"""
    n = 300
    rng = np.random.default_rng(23)
    x = rng.uniform(0., 5., (n, 2))
    s = rng.uniform(0.01, 2., n)
    y = 5. * np.sin(x).sum(axis=1) + 5. * np.sqrt(s) * rng.standard_normal(n)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.3, 0.9) + ab.IndependentNoise(0.2), context=ctx)
    indexer = ragged_groups()
    K = orc.gram(model.covariance_function_, x, x_meas=True) + np.diag(s)
    blocks = logo_marginal_closed_form(K, y, s, list(indexer.values()))[4]
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
    metric = ab.LeaveOneGroupOutLikelihood(indexer, "marginal")
    assert metric.group_scores(_dataset(x, y, s), _m52(ctx))["empty"] == 0.
    assert ab.LeaveOneGroupOutLikelihood({}, "marginal")(_dataset(x, y, s), _m52(ctx)) == 0.
    assert ab.LeaveOneGroupOutLikelihood({}, "marginal").group_scores(_dataset(x, y, s), _m52(ctx)) == {}


def test_size_class_split_into_two_chunks(ctx):
    """60 groups of 2 and 60 of 3 are one size class, but padded to 3 they are 360 columns, more than the n = 300 a chunk
    may hold: the class advances as two chunks, whose terms and blocks must land where one chunk's would"""
    n = 300
    x, y = _data(n, 3, 77)
    perm = np.random.default_rng(78).permutation(n)
    indexer = {g: perm[3 * g:3 * g + 3].tolist() for g in range(60)}
    indexer.update({60 + g: perm[180 + 2 * g:182 + 2 * g].tolist() for g in range(60)})
    check(_m52(ctx), x, y, _variance(n, 79), indexer, brute=True)


class _Raw:
    """one problem of n points for direct calls of the typed entry"""

    def __init__(self, ctx, n=60):
        self.ctx = ctx
        self.x, self.y = _data(n, 2, 6)
        self.s = _variance(n, 2)
        self.cov = ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1)  # nodes: 0 SE, 1 noise, 2 sum
        self.fs = self.cov.features(self.x)
        self.struct = self.fs.as_struct()
        self.n = n

    def call(self, offsets, indices, predict_type=capi.PREDICT_MARGINAL, slots=((0, 0), (0, 1), (1, 0)), struct=None, y=None,
             s=None, weights=True):
        """(status, value, grad, u, group_nll); every output starts at -7"""
        offsets, indices = np.asarray(offsets, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        table = (capi.GradientSlot * max(1, len(slots)))(*[capi.GradientSlot(a, b) for a, b in slots])
        value = C.c_double(-7.)
        grad, u, terms = np.full(max(1, len(slots)), -7.), np.full(self.n, -7.), np.full(max(1, len(offsets) - 1), -7.)
        st = self.ctx._lib.agp_logo_nll_gradient_typed(self.ctx._h, self.ctx.kernel(self.cov), C.byref(struct or self.struct),
                                                       y or _p(self.y), s or _p(self.s), len(offsets) - 1, _p(offsets), _p(indices),
                                                       predict_type, len(slots), table, None, 0, C.byref(value), _p(grad),
                                                       _p(u) if weights else None, _p(terms))
        return st, value.value, grad, u, terms

    def call_untyped(self, offsets, indices, slots=((0, 0), (0, 1), (1, 0))):
        offsets, indices = np.asarray(offsets, dtype=np.int64), np.asarray(indices, dtype=np.int64)
        table = (capi.GradientSlot * max(1, len(slots)))(*[capi.GradientSlot(a, b) for a, b in slots])
        value = C.c_double(-7.)
        grad, u = np.full(max(1, len(slots)), -7.), np.full(self.n, -7.)
        st = self.ctx._lib.agp_logo_nll_gradient(self.ctx._h, self.ctx.kernel(self.cov), C.byref(self.struct), _p(self.y), _p(self.s),
                                                 len(offsets) - 1, _p(offsets), _p(indices), len(slots), table, None, 0,
                                                 C.byref(value), _p(grad), _p(u))
        return st, value.value, grad, u


def _flat(indexer):
    groups = [np.asarray(g, dtype=np.int64) for g in indexer.values()]
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    indices = np.concatenate(groups).astype(np.int64) if groups else np.zeros(0, dtype=np.int64)
    return groups, offsets, indices


@pytest.mark.parametrize("predict_type", ["joint", "marginal"])
def test_group_nll_in_the_callers_order(ctx, predict_type):
    """an indexer whose sizes are not sorted, with empty groups: the device orders its terms by size, the entry hands them
    back in the caller's order, 0 for the empty groups, from the value-only and from the gradient call"""
    raw = _Raw(ctx, n=300)
    perm = np.random.default_rng(5).permutation(300)
    sizes = [7, 130, 0, 1, 33, 2, 0, 65, 3, 17, 1, 16]
    edges = np.concatenate([[0], np.cumsum(sizes)])
    indexer = {f"g{g:02d}": perm[edges[g]:edges[g + 1]].tolist() for g in range(len(sizes))}
    groups, offsets, indices = _flat(indexer)
    K = orc.gram(raw.cov, raw.x, x_meas=True) + np.diag(raw.s)
    if predict_type == "marginal":
        value, _, _, _, _, terms = logo_marginal_closed_form(K, raw.y, raw.s, groups)
    else:
        value = logo_closed_form(K, raw.y, raw.s, groups)[0]
        terms = [logo_closed_form(K, raw.y, raw.s, [g])[0] for g in groups]
    ptype = capi.PREDICT_MARGINAL if predict_type == "marginal" else capi.PREDICT_JOINT
    full = raw.call(offsets, indices, ptype)
    alone = raw.call(offsets, indices, ptype, slots=(), weights=False)
    for st, logo, _, _, got in (full, alone):
        assert st == capi.AGP_OK
        assert abs(logo - value) <= 1e-10 * abs(value), (logo, value)
        for g, (a, b) in enumerate(zip(got, terms)):
            assert abs(a - b) <= 1e-10 * max(1., abs(b)), (g, a, b)
        assert got[2] == 0. and got[6] == 0.
        assert abs(got.sum() - logo) <= 1e-12 * abs(logo), (got.sum(), logo)
    model = ab.gp_from_covariance(raw.cov, context=ctx)
    scores = ab.LeaveOneGroupOutLikelihood(indexer, predict_type).group_scores(_dataset(raw.x, raw.y, raw.s), model)
    assert list(scores) == list(indexer)
    assert np.array(list(scores.values())).tobytes() == alone[4].tobytes()


def test_joint_through_the_typed_entry_is_the_untyped_entry_and_marginal_is_deterministic(ctx):
    raw = _Raw(ctx, n=300)
    _, offsets, indices = _flat(ragged_groups(seed=4))
    old = raw.call_untyped(offsets, indices)
    new = raw.call(offsets, indices, capi.PREDICT_JOINT)
    assert old[0] == capi.AGP_OK and new[0] == capi.AGP_OK
    assert old[1] == new[1] and old[2].tobytes() == new[2].tobytes() and old[3].tobytes() == new[3].tobytes()
    old = raw.call_untyped(offsets, indices, slots=())
    new = raw.call(offsets, indices, capi.PREDICT_JOINT, slots=())
    assert old[0] == capi.AGP_OK and old[1] == new[1] and old[3].tobytes() == new[3].tobytes()
    m1, m2 = raw.call(offsets, indices), raw.call(offsets, indices)
    assert m1[0] == capi.AGP_OK and m1[1] == m2[1] and m1[1] != new[1]
    assert all(m1[i].tobytes() == m2[i].tobytes() for i in (2, 3, 4))
    v1, v2 = raw.call(offsets, indices, slots=(), weights=False), raw.call(offsets, indices, slots=(), weights=False)
    assert v1[0] == capi.AGP_OK and v1[1] == v2[1] and v1[4].tobytes() == v2[4].tobytes()


def test_malformed_calls_write_nothing(ctx):
    raw = _Raw(ctx)
    n = raw.n
    good = (np.array([0, 3, 3, 10]), np.array([5, 1, 9, 20, 21, 22, 23, 24, 25, 59]))
    st, value, grad, u, terms = raw.call(*good)
    assert st == capi.AGP_OK and value != -7. and np.all(grad[:3] != -7.) and np.all(u != -7.)
    assert terms[1] == 0. and np.all(terms != -7.)

    def refused(offsets, indices, predict_type=capi.PREDICT_MARGINAL, slots=((0, 0), (0, 1), (1, 0))):
        st, value, grad, u, terms = raw.call(offsets, indices, predict_type, slots)
        assert st == capi.AGP_ERR_INVALID_ARGUMENT
        assert value == -7. and np.all(grad == -7.) and np.all(u == -7.) and np.all(terms == -7.)

    refused(*good, predict_type=2)                                   # an unknown predict type
    refused(*good, predict_type=-1)
    refused([0, 3, 3, 10], [5, 1, 5, 20, 21, 22, 23, 24, 25, 59])    # an index twice in one group
    refused([0, 3, 3, 10], [5, 1, 9, 20, 21, 22, 23, 24, 9, 59])     # an index in two groups
    refused([0, 3, 3, 10], [5, 1, 9, 20, 21, 22, 23, 24, 25, n])     # out of range
    refused([0, 3, 3, 10], [5, 1, 9, 20, 21, -1, 23, 24, 25, 59])
    refused([1, 3, 3, 10], good[1])                                  # offsets[0] != 0
    refused([0, 3, 2, 10], good[1])                                  # offsets not monotone
    refused(*good, slots=((2, 0),))                                  # the sum node
    refused(*good, slots=((0, 2),))                                  # a radial leaf has two parameters
    refused(*good, slots=((0, 0),) * (capi.MAX_GRADIENT_SLOTS + 1))


def test_errors(ctx):
    x, _ = _data(20, 2, 4)
    xd = np.concatenate([x[:10], x[:10]])
    indexer = {0: list(range(10)), 1: list(range(10, 20))}
    bad = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0), context=ctx)
    with pytest.raises(ab.NotPositiveDefiniteError):
        bad.leave_one_group_out_likelihood_gradient(ab.RegressionDataset(xd, np.zeros(20)), indexer, predict_type="marginal")
    # ... and through the entry: the status code, nothing written
    cov = bad.covariance_function_
    struct = cov.features(xd).as_struct()
    offsets, indices = np.array([0, 10, 20], dtype=np.int64), np.arange(20, dtype=np.int64)
    value, terms, zeros = C.c_double(-7.), np.full(2, -7.), np.zeros(20)
    st = ctx._lib.agp_logo_nll_gradient_typed(ctx._h, ctx.kernel(cov), C.byref(struct), _p(zeros), None, 2, _p(offsets), _p(indices),
                                              capi.PREDICT_MARGINAL, 0, None, None, 0, C.byref(value), None, None, _p(terms))
    assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and value.value == -7. and np.all(terms == -7.)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    with pytest.raises(ValueError):
        model.leave_one_group_out_likelihood_gradient(ab.RegressionDataset(x, np.zeros(20)), indexer, predict_type="diagonal")
    with pytest.raises(ValueError):
        ab.LeaveOneGroupOutLikelihood(indexer, "diagonal")


def test_device_resident_inputs_equal_host_inputs(ctx):
    raw = _Raw(ctx, n=300)
    _, offsets, indices = _flat(ragged_groups(seed=6))
    host = raw.call(offsets, indices)
    assert host[0] == capi.AGP_OK
    keep = [ctx.to_device(np.ravel(raw.fs.coords, order="K")), ctx.to_device(raw.y), ctx.to_device(raw.s)]
    struct = raw.cov.features(raw.x).as_struct()
    struct.coords = keep[0].ptr
    assert raw.fs.scales is None
    struct.location = capi.DEVICE
    dev = raw.call(offsets, indices, struct=struct, y=C.c_void_p(keep[1].ptr), s=C.c_void_p(keep[2].ptr))
    assert dev[0] == capi.AGP_OK
    assert host[1] == dev[1] and all(host[i].tobytes() == dev[i].tobytes() for i in (2, 3, 4))
    for d in keep:
        d.free()


def test_cpp_logo_marginal_matches_python(ctx):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "logo_marginal_check")], text=True)
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

    logo, grad = model.leave_one_group_out_likelihood_gradient(ds, station, predict_type="marginal")
    joint, _ = model.leave_one_group_out_likelihood_gradient(ds, station)
    assert abs(logo - joint) > 1e-6 * abs(joint)
    metric = ab.LeaveOneGroupOutLikelihood(station, "marginal")
    cpp = {k[len("grad_"):]: float(v[0][0]) for k, v in rows.items() if k.startswith("grad_")}
    assert set(cpp) == set(grad)
    assert abs(float(rows["logo_nll"][0][0]) - logo) <= 1e-10 * abs(logo)
    assert abs(float(rows["logo_nll_metric"][0][0]) - metric(ds, model)) <= 1e-10 * abs(logo)
    for name in grad:
        assert abs(cpp[name] - grad[name]) <= 1e-10 * max(abs(grad[name]), 1e-3 * max(abs(g) for g in grad.values())), name
    scores = metric.group_scores(ds, model)
    cpp_scores = {k[len("group_"):]: float(v[0][0]) for k, v in rows.items() if k.startswith("group_")}
    assert list(cpp_scores) == list(scores) and len(scores) == 10
    for key, t in scores.items():
        assert abs(cpp_scores[key] - t) <= 1e-10 * max(1., abs(t)), key
    loo = ab.LeaveOneOutLikelihood()(ds, model)
    assert rows["loo_nll_joint"] == rows["loo_nll_marginal"]
    assert abs(float(rows["loo_nll_marginal"][0][0]) - loo) <= 1e-10 * abs(loo)
