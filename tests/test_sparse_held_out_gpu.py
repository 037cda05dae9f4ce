"""GPU tests of the sparse model's leave-one-group-out cross validation from one fit: agp_sparse_held_out and, on
SparseGaussianProcessRegression, held_out_predictions, cross_validate, leave_one_group_out_likelihood and group_scores.

Reference: the numpy closed form of tests/sparse_held_out_cases.py (which tests/test_sparse_held_out_host.py checks against
real leave-group-out refits) on the oracle's Gram matrices.  Bounds, those of the sparse path (tests/test_sparse_gp_gpu.py,
tests/test_sparse_gradient_gpu.py): means to 1e-8 max(1, max|mean|), variances and joint blocks to 1e-8 max|cov_g|, the
metric to 1e-8 n, each group term to 1e-8 max(1, |g|).  Every case first asserts its input conditions on the reference
side: cond(K_uu) <= 1e6, cond(Kt) <= 1e6, cond(V_g) <= 1e4.  Each check prints its worst measured ratio to the bound.

Shapes, the smallest that cross every edge (the layouts follow the rule of sparse_api.hip's sparse_observations): two groups
of 130 (lock step, a group wider than one 128 panel), 64 groups of 4 (lock step, many small blocks in one chunk), 13 ragged
sizes on both sides of each power of two (padded slabs, several size classes), 35 sizes with 26 singletons (one fit per
block)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from oracle import oracle_py as orc
from sparse_held_out_cases import INDUCING_NUGGET, LENGTH, MEASUREMENT_NUGGET, NOISE, SHAPES, SIGMA, closed_form, problem_1d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _cov_1d():
    return ab.SquaredExponential(LENGTH, SIGMA) + ab.measurement_only(ab.IndependentNoise(NOISE))


def _model(ctx, cov, x, keys, u, mn, inn, mean=None):
    lookup = {np.asarray(f, dtype=np.float64).tobytes(): int(k) for f, k in zip(x, keys)}
    grouper = lambda f: lookup[np.asarray(f, dtype=np.float64).tobytes()]
    if mean is None:
        model = ab.sparse_gp_from_covariance(cov, grouper, ab.FixedInducingPoints(u), "sparse", context=ctx)
    else:
        model = ab.sparse_gp_from_covariance_and_mean(cov, mean, grouper, ab.FixedInducingPoints(u), "sparse", context=ctx)
    model.set_param("measurement_nugget", mn)
    model.set_param("inducing_nugget", inn)
    return model


def _reference(cov, x, y, yvar, offsets, u, mn, inn):
    """closed_form on the oracle's Gram matrices, with the input conditions asserted"""
    n = len(y)
    Kmm, Kpp = orc.gram(cov, x, x_meas=True), orc.gram(cov, x)
    Kfu = orc.gram(cov, x, u, x_meas=True)
    Kuu = orc.gram(cov, u) + inn * np.eye(len(u))
    cf = closed_form(Kmm, Kpp, Kfu, Kuu, np.zeros(n) if yvar is None else yvar, mn, offsets, y)
    assert cf["cond_Kuu"] <= 1e6 and cf["cond_Kt"] <= 1e6 and max(cf["cond_V"]) <= 1e4, (cf["cond_Kuu"], cf["cond_Kt"], max(cf["cond_V"]))
    return cf


def _case_1d(shape):
    """(cov, x, y, yvar, offsets, keys, u, reference), computed once per shape and left unchanged"""
    if shape not in _CACHE:
        x, y, yvar, offsets, u = problem_1d(shape)
        cov = _cov_1d()
        keys = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
        _CACHE[shape] = (cov, x, y, yvar, offsets, keys, u, _reference(cov, x, y, yvar, offsets, u, MEASUREMENT_NUGGET, INDUCING_NUGGET))
    return _CACHE[shape]


def _case_3d():
    """the ragged_3d recipe of tests/sparse_gradient_cases.py cut to 300 points: Matern-5/2, no target variances,
    inducing points not on the data"""
    if "3d" not in _CACHE:
        rng = np.random.default_rng(11)
        n, m = 300, 45
        x = rng.uniform(0., 20., (n, 3))
        y = np.sin(x[:, 0]) + 0.3 * x[:, 0] + 0.1 * rng.standard_normal(n)
        cov = ab.Matern52(4.0, 2.0) + ab.measurement_only(ab.IndependentNoise(0.2))
        keys = np.floor(x[:, 0] / 1.7).astype(np.int64)
        u = rng.uniform(0., 20., (m, 3))
        order = np.argsort(keys, kind="stable")
        uniq, counts = np.unique(keys, return_counts=True)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        ref = _reference(cov, x[order], y[order], None, offsets, u, 1e-10, 1e-6)
        _CACHE["3d"] = (cov, x, y, keys, u, order, offsets, [int(k) for k in uniq], ref)
    return _CACHE["3d"]


def _check_predictions(label, held, keys, ref, mean_shift=None):
    worst_mean = worst_cov = 0.
    for g, key in enumerate(keys):
        p = held[key]
        want = ref["mean"][g] + (0. if mean_shift is None else mean_shift[g])
        worst_mean = max(worst_mean, np.abs(p.mean - want).max() / (1e-8 * max(1., np.abs(want).max())))
        worst_cov = max(worst_cov, np.abs(p.covariance - ref["cov"][g]).max() / (1e-8 * np.abs(ref["cov"][g]).max()))
    print(f"{label}: mean {worst_mean:.2e} of its bound, joint blocks {worst_cov:.2e} of theirs")
    assert worst_mean <= 1. and worst_cov <= 1.


def _check_scores(label, value, scores, ref, which, n, sizes):
    terms = np.asarray(ref[which])
    ratio_value = abs(value - terms.sum()) / (1e-8 * n)
    ratio_terms = max(abs(s - t) / (1e-8 * max(1., sz)) for s, t, sz in zip(scores.values(), terms, sizes))
    print(f"{label} {which}: metric {ratio_value:.2e} of its bound, group terms {ratio_terms:.2e} of theirs")
    assert ratio_value <= 1. and ratio_terms <= 1.


@pytest.mark.parametrize("predict_type", ["joint", "marginal"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_metric_and_group_scores_match_closed_form(ctx, shape, predict_type):
    cov, x, y, yvar, offsets, keys, u, ref = _case_1d(shape)
    model = _model(ctx, cov, x, keys, u, MEASUREMENT_NUGGET, INDUCING_NUGGET)
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, yvar))
    value = model.leave_one_group_out_likelihood(ds, predict_type)
    scores = model.group_scores(ds, predict_type)
    assert list(scores) == list(range(len(offsets) - 1))
    _check_scores(shape, value, scores, ref, "nll_" + predict_type, len(x), np.diff(offsets))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_held_out_predictions_match_closed_form(ctx, shape):
    cov, x, y, yvar, offsets, keys, u, ref = _case_1d(shape)
    model = _model(ctx, cov, x, keys, u, MEASUREMENT_NUGGET, INDUCING_NUGGET)
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, yvar))
    held = model.held_out_predictions(ds)
    assert list(held) == list(range(len(offsets) - 1))
    _check_predictions(shape, held, list(held), ref)
    # the marginal surface of cross_validate(): the same means, the diagonals of the blocks
    cv = model.cross_validate().predict(ds)
    marg = cv.marginals()
    worst = max(np.abs(marg[k].covariance - np.diag(ref["cov"][g])).max() / (1e-8 * np.abs(ref["cov"][g]).max()) for g, k in enumerate(held))
    print(f"{shape}: variances {worst:.2e} of their bound")
    assert worst <= 1.
    full = cv.marginal()
    assert np.array_equal(full.mean, np.concatenate([marg[k].mean for k in held]))  # (x is in grouped order already)


def test_joint_and_marginal_differ(ctx):
    """the diagonal path really ran: the two predict types are different numbers"""
    cov, x, y, yvar, offsets, keys, u, ref = _case_1d("ragged_13")
    model = _model(ctx, cov, x, keys, u, MEASUREMENT_NUGGET, INDUCING_NUGGET)
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, yvar))
    joint, marginal = model.leave_one_group_out_likelihood(ds, "joint"), model.leave_one_group_out_likelihood(ds, "marginal")
    assert abs(joint - marginal) > 1e-3 * abs(joint)
    assert abs(sum(ref["nll_joint"]) - sum(ref["nll_marginal"])) > 1e-3 * abs(sum(ref["nll_joint"]))


def test_matern_3d_without_variances_with_linear_mean(ctx):
    cov, x, y, keys, u, order, offsets, uniq, ref = _case_3d()
    mean = ab.LinearMean(0.3, -0.2)
    model = _model(ctx, cov, x, keys, u, 1e-10, 1e-6, mean=mean)
    ds = ab.RegressionDataset(x, y)  # (NOT in grouped order: the model reorders)
    held = model.held_out_predictions(ds)
    assert list(held) == uniq
    xs = x[order]
    shift = [mean(xs[offsets[g]:offsets[g + 1]]) for g in range(len(uniq))]  # the mean function is added back
    _check_predictions("matern 3-D", held, uniq, ref, shift)
    for predict_type in ("joint", "marginal"):
        _check_scores("matern 3-D", model.leave_one_group_out_likelihood(ds, predict_type), model.group_scores(ds, predict_type), ref,
                      "nll_" + predict_type, len(x), np.diff(offsets))
    # cross_validate().predict(...).mean() comes back in the order of the data set
    cv_mean = model.cross_validate().predict(ds).mean()
    want = np.empty(len(x))
    want[order] = np.concatenate([ref["mean"][g] + shift[g] for g in range(len(uniq))])
    assert np.abs(cv_mean - want).max() <= 1e-8 * max(1., np.abs(want).max())


def test_agrees_with_the_library_refits(ctx):
    """fit(rest).predict(x_g).joint() with FixedInducingPoints for the largest group, a middle one and the singleton:
    two device routes, each good to 1e-8"""
    cov, x, y, yvar, offsets, keys, u, ref = _case_1d("ragged_13")
    model = _model(ctx, cov, x, keys, u, MEASUREMENT_NUGGET, INDUCING_NUGGET)
    held = model.held_out_predictions(ab.RegressionDataset(x, ab.MarginalDistribution(y, yvar)))
    for g in (0, 5, 12):
        rest = keys != g
        refit = model.fit(ab.RegressionDataset(x[rest], ab.MarginalDistribution(y[rest], yvar[rest]))).predict(x[~rest]).joint()
        em = np.abs(held[g].mean - refit.mean).max() / max(1., np.abs(refit.mean).max())
        ec = np.abs(held[g].covariance - refit.covariance).max() / np.abs(refit.covariance).max()
        print(f"group {g} (size {np.sum(~rest)}): mean {em:.2e}, covariance {ec:.2e} against the refit")
        assert em <= 1e-7 and ec <= 1e-7


class _Raw:
    """agp_sparse_held_out through ctypes for the 13-group problem"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.cov, self.x, self.y, self.yvar, self.offsets, _, self.u, _ = _case_1d("ragged_13")
        self.fx, self.fu = self.cov.features(self.x), self.cov.features(self.u)
        self.n, self.G = len(self.x), len(self.offsets) - 1

    def call(self, offsets=None, predict_type=capi.PREDICT_JOINT, everything=True, n_groups=None):
        offsets = self.offsets if offsets is None else np.asarray(offsets, dtype=np.int64)
        sx, su = self.fx.as_struct(), self.fu.as_struct()
        value = C.c_double(-7.)
        sizes = np.diff(self.offsets)
        terms, mean, var, joint = np.full(self.G, -7.), np.full(self.n, -7.), np.full(self.n, -7.), np.full(int(np.sum(sizes * sizes)), -7.)
        st = self.ctx._lib.agp_sparse_held_out(self.ctx._h, self.ctx.kernel(self.cov), C.byref(sx), self.G if n_groups is None else n_groups,
                                               _p(offsets), _p(self.y), _p(self.yvar), C.byref(su), MEASUREMENT_NUGGET, INDUCING_NUGGET,
                                               predict_type, C.byref(value), *([_p(terms), _p(mean), _p(var), _p(joint)] if everything else [None] * 4))
        return st, value.value, terms, mean, var, joint


def test_group_scores_sum_and_bitwise_repeatability(ctx):
    raw = _Raw(ctx)
    for ptype in (capi.PREDICT_JOINT, capi.PREDICT_MARGINAL):
        full, again, only = raw.call(predict_type=ptype), raw.call(predict_type=ptype), raw.call(predict_type=ptype, everything=False)
        assert full[0] == again[0] == only[0] == capi.AGP_OK
        assert full[1] == again[1] and all(full[i].tobytes() == again[i].tobytes() for i in (2, 3, 4, 5))  # two identical calls
        assert only[1] == full[1]  # the metric alone, bit for bit
        assert abs(full[2].sum() - full[1]) <= 1e-12 * abs(full[1])
        assert not np.any(full[5] == -7.) and not np.any(full[3] == -7.)


def test_errors(ctx):
    raw = _Raw(ctx)
    bad = raw.offsets.copy()
    bad[3], bad[4] = bad[4], bad[3]  # (not monotone)
    shifted = raw.offsets.copy()
    shifted[0] = 1
    short = raw.offsets.copy()
    short[-1] -= 1
    for kwargs in ({"offsets": bad}, {"offsets": shifted}, {"offsets": short}, {"predict_type": 2}, {"predict_type": -1}, {"n_groups": 0}):
        st, value, terms, mean, var, joint = raw.call(**kwargs)
        assert st == capi.AGP_ERR_INVALID_ARGUMENT, kwargs
        assert value == -7. and all(np.all(a == -7.) for a in (terms, mean, var, joint)), kwargs  # nothing is written
    cov, x, y, yvar, offsets, keys, u, _ = _case_1d("ragged_13")
    model = _model(ctx, cov, x, keys, u, MEASUREMENT_NUGGET, INDUCING_NUGGET)
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, yvar))
    with pytest.raises(ValueError, match="own groups"):
        model.cross_validate().predict(ds, lambda f: int(f // 7.))
    with pytest.raises(ValueError, match="predict_type"):
        model.leave_one_group_out_likelihood(ds, "both")
    xn = x.copy()
    xn[17] = np.nan
    lookup_model = ab.sparse_gp_from_covariance(cov, lambda f: 0 if not f == f else int(f > 15.), ab.FixedInducingPoints(u), "sparse", context=ctx)
    with pytest.raises(ab.NanInputError):
        lookup_model.leave_one_group_out_likelihood(ab.RegressionDataset(xn, ab.MarginalDistribution(y, yvar)))


def test_cpp_sparse_logo_matches_python(ctx):
    ex = os.path.join(ROOT, "examples")
    subprocess.check_call(["make", "-s", "-C", ex])
    out = subprocess.check_output([os.path.join(ex, "sparse_logo_check")], text=True)
    rows = {}
    for line in out.strip().splitlines():
        key, *vals = line.split(",")
        rows.setdefault(key, []).append(vals)
    data = np.array(rows["x"], dtype=float)
    x, y, var = data[:, 1:4], data[:, 4], data[:, 5]
    cov = ab.Matern52(2.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.2))
    model = ab.sparse_gp_from_covariance(cov, lambda f: int(np.floor(f[0] / 1.3)), ab.FixedInducingPoints(x[::10]), "sparse", context=ctx)
    model.set_param("inducing_nugget", 1e-6)
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, var))
    for ptype in ("joint", "marginal"):
        value = model.leave_one_group_out_likelihood(ds, ptype)
        assert abs(float(rows["logo_" + ptype][0][0]) - value) <= 1e-10 * abs(value)
        scores = model.group_scores(ds, ptype)
        cpp = {int(k[len("group_" + ptype + "_"):]): float(v[0][0]) for k, v in rows.items() if k.startswith("group_" + ptype + "_")}
        assert sorted(cpp) == list(scores) and len(scores) >= 7
        for key, t in scores.items():
            assert abs(cpp[key] - t) <= 1e-10 * max(1., abs(t)), key
    p = model.held_out_predictions(ds)[3]
    held = np.array(rows["held"], dtype=float)
    assert int(rows["held_size"][0][0]) == p.size() == len(held)
    assert np.abs(held[:, 1] - p.mean).max() <= 1e-10 * max(1., np.abs(p.mean).max())
    assert np.abs(held[:, 2] - np.diag(p.covariance)).max() <= 1e-10 * np.abs(p.covariance).max()
    assert np.abs(held[:, 3] - p.covariance[:, 0]).max() <= 1e-10 * np.abs(p.covariance).max()
