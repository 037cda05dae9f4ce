"""agp_predict_batch (include/albatross_amd.h; csrc/predict_batch.hip) and ab.predict_batch: the predictions of B fits of one
size in lock step - against the oracle and the per-fit predict() loop at the edges of every kernel on the path (the
128-row panels and 512-row outer blocks of the substitution, the 32 columns of the covariance tile, the 64 columns of the
substitution's micro-kernel), with uniform and mixed trees, measurement-wrapped test points, mean functions, fits of mixed
origin, a failed fit in the batch, malformed arguments and device-resident outputs.

Bounds: the ones the project holds predictions from batch fits to (tests/test_fit_batch_gpu.py) - mean 1e-8 max|ref|,
variance and covariance 1e-8 max|ref| + 1e-9."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from oracle import oracle_py as orc

pytestmark = pytest.mark.gpu

WHATS = ("mean", "marginal", "joint")


def _problems(n, count, seed, with_variance, same_tree=False):
    rng = np.random.default_rng(seed)
    covs, data = [], []
    for b in range(count):
        x = rng.uniform(0., 10., (n, 3))
        y = np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) + 0.05 * b
        yvar = rng.uniform(0.01, 0.05, n) if with_variance and b % 2 == 0 else None
        if yvar is not None:
            x[5] = x[2]  # duplicate point: IndependentNoise fires off the diagonal too (the target variance keeps K definite)
        if same_tree:
            cov = ab.Matern52(1.5 + 0.02 * b, 1.0) + ab.IndependentNoise(0.1 + 0.002 * b)
        else:  # different parameter vectors AND different trees across the batch
            cov = (ab.Matern52(1.5 + 0.25 * b, 1.0) if b % 3 else ab.SquaredExponential(1.0 + 0.1 * b, 1.2)) + ab.IndependentNoise(0.1 + 0.01 * b)
        covs.append(cov)
        data.append((x, y, yvar))
    return covs, data


def _fit(ctx, covs, data, means=None):
    models = [ab.gp_from_covariance(c, context=ctx) if not means or means[b] is None else ab.gp_from_covariance_and_mean(c, means[b], context=ctx)
              for b, c in enumerate(covs)]
    datasets = [ab.RegressionDataset(x, y if v is None else ab.MarginalDistribution(y, v)) for x, y, v in data]
    return models, datasets, ab.fit_batch(models, datasets)


def _close(got, ref, absolute, what):
    err, bound = np.abs(np.asarray(got) - np.asarray(ref)).max(), 1e-8 * np.abs(ref).max() + absolute
    print(f"{what}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def _check(pred, ref, what, label):
    """pred: an entry of predict_batch's result; ref: (mean,), (mean, variance) or (mean, covariance)"""
    if what == "mean":
        _close(pred, ref[0], 0., f"{label} mean")
    else:
        _close(pred.mean, ref[0], 0., f"{label} {what} mean")
        _close(pred.covariance, ref[1], 1e-9, f"{label} {what} second moment")


def _oracle(ofit, xs, what, xs_meas=False):
    if what == "mean":
        return (ofit.predict_mean(xs, xs_meas),)
    return ofit.predict_marginal(xs, xs_meas) if what == "marginal" else ofit.predict_joint(xs, xs_meas)


def _single(fm, xs, what):
    p = fm.predict(xs)
    if what == "mean":
        return (p.mean(),)
    d = p.marginal() if what == "marginal" else p.joint()
    return d.mean, d.covariance


# n: below one 128-row panel, exactly one, one more row, exactly one 512-row outer block, a partial panel past it;
# m: one column, either side of the covariance tile's 32 and of the micro-kernel's 64 columns, several tiles;
# count 1 (a run of one: the single path), 2, 5; trees mixed (the generator alternates them) except where noted
@pytest.mark.parametrize("n,count,m,with_variance,same_tree", [
    (100, 5, 200, False, False),
    (128, 2, 31, True, False),
    (129, 1, 33, False, False),
    (129, 2, 1, False, False),
    (512, 2, 64, True, False),
    (700, 2, 65, True, False),
    (256, 40, 33, False, True),  # uniform trees: every covariance launch is ONE launch for the batch
])
def test_predict_batch_matches_oracle_and_single_predictions(ctx, n, count, m, with_variance, same_tree):
    covs, data = _problems(n, count, n + count + m, with_variance, same_tree)
    models, datasets, fms = _fit(ctx, covs, data)
    rng = np.random.default_rng(3)
    xs = [rng.uniform(0., 10., (m, 3)) for _ in range(count)]
    ofits = [orc.OracleFit(cov, x, y, v) for cov, (x, y, v) in zip(covs, data)]
    for what in WHATS:
        preds = ab.predict_batch(fms, xs, what=what)
        assert len(preds) == count
        for b in range(count):
            _check(preds[b], _oracle(ofits[b], xs[b], what), what, f"n={n} m={m} problem {b} vs oracle")
            _check(preds[b], _single(fms[b], xs[b], what), what, f"n={n} m={m} problem {b} vs predict()")
        if what == "joint":
            for p in preds:
                assert np.array_equal(p.covariance, p.covariance.T)  # the full symmetric matrix, mirrored bit for bit
    # one array shared by every problem
    shared = ab.predict_batch(fms, xs[0], what="marginal")
    _check(shared[-1], _single(fms[-1], xs[0], "marginal"), "marginal", "shared features")


def test_predict_batch_past_two_outer_blocks_matches_single_predictions(ctx):
    n, count, m = 1300, 4, 65
    covs, data = _problems(n, count, 17, True)
    _, _, fms = _fit(ctx, covs, data)
    xs = [np.random.default_rng(b).uniform(0., 10., (m, 3)) for b in range(count)]
    for what in WHATS:
        preds = ab.predict_batch(fms, xs, what=what)
        for b in range(count):
            _check(preds[b], _single(fms[b], xs[b], what), what, f"n={n} problem {b} vs predict()")


def test_measurement_wrapped_test_features(ctx):
    """problem 1 predicts AT training points: the noise term fires in the cross covariance and in the prior"""
    n, count, m = 200, 3, 40
    covs, data = _problems(n, count, 23, False)
    _, _, fms = _fit(ctx, covs, data)
    rng = np.random.default_rng(4)
    xs = [rng.uniform(0., 10., (m, 3)) for _ in range(count)]
    xs[1] = data[1][0][:m].copy()
    for what in WHATS:
        preds = ab.predict_batch(fms, [ab.Measurement(x) for x in xs], what=what)
        for b in range(count):
            ofit = orc.OracleFit(covs[b], *data[b])
            _check(preds[b], _oracle(ofit, xs[b], what, xs_meas=True), what, f"measurement problem {b} vs oracle")
    plain = ab.predict_batch(fms, xs, what="marginal")
    noisy = ab.predict_batch(fms, [ab.Measurement(x) for x in xs], what="marginal")
    assert np.all(noisy[1].covariance >= plain[1].covariance)


def test_mean_functions_are_added_back_per_model(ctx):
    n, count, m = 150, 3, 20
    rng = np.random.default_rng(31)
    covs = [ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1) for _ in range(count)]
    data = [(x, 0.7 * x[:, 0] - 1.0 + np.sin(x).sum(axis=1), None) for x in (rng.uniform(0., 10., (n, 1)) for _ in range(count))]
    means = [None, ab.LinearMean(0.6, -0.8), None]
    _, _, fms = _fit(ctx, covs, data, means)
    xs = rng.uniform(0., 10., (m, 1))
    for what in WHATS:
        preds = ab.predict_batch(fms, xs, what=what)
        for b in range(count):
            ofit = orc.OracleFit(covs[b], data[b][0], data[b][1], mean=means[b])
            _check(preds[b], _oracle(ofit, xs, what), what, f"mean function problem {b} vs oracle")
            _check(preds[b], _single(fms[b], xs, what), what, f"mean function problem {b} vs predict()")


def _bits(preds, what):
    if what == "mean":
        return [p.tobytes() for p in preds]
    return [(p.mean.tobytes(), np.ascontiguousarray(p.covariance).tobytes()) for p in preds]


@pytest.mark.parametrize("same_tree", [True, False])
def test_deterministic_and_independent_of_position(ctx, same_tree):
    n, m = 300, 40
    covs, data = _problems(n, 8, 41, True, same_tree)
    _, _, fms = _fit(ctx, covs, data)
    xs = [np.random.default_rng(b).uniform(0., 10., (m, 3)) for b in range(8)]
    for what in WHATS:
        whole = _bits(ab.predict_batch(fms, xs, what=what), what)
        assert _bits(ab.predict_batch(fms, xs, what=what), what) == whole
        part = _bits(ab.predict_batch(fms[2:6], xs[2:6], what=what), what)
        assert part == whole[2:6]
        # an evenly spaced subset is a run too
        assert _bits(ab.predict_batch(fms[1::2], xs[1::2], what=what), what) == whole[1::2]


@pytest.mark.parametrize("same_tree", [True, False])
def test_sub_batches_give_the_bits_of_one_pass(make_ctx, monkeypatch, same_tree):
    """AGP_PREDICT_CHUNK=100 with m = 33 holds 3 problems per sub-batch: a run of 8 goes as 3 + 3 + 2 (table entries,
    factor offsets, the joint prior's table and the workspace are indexed per sub-batch) - same bits as one pass, and the
    per-fit loop within the bounds"""
    n, m, count = 200, 33, 8
    covs, data = _problems(n, count, 61, True, same_tree)
    xs = [np.random.default_rng(b).uniform(0., 10., (m, 3)) for b in range(count)]
    bits = []
    for chunk in ("0", "100"):
        monkeypatch.setenv("AGP_PREDICT_CHUNK", chunk)
        ctx = make_ctx()  # (the switch is read when the context is created)
        _, _, fms = _fit(ctx, covs, data)
        per_mode = []
        for what in WHATS:
            preds = ab.predict_batch(fms, xs, what=what)
            per_mode.append(_bits(preds, what))
            if chunk != "0":
                for b in range(count):
                    _check(preds[b], _single(fms[b], xs[b], what), what, f"sub-batch problem {b} vs predict()")
        bits.append(per_mode)
        del fms
    assert bits[0] == bits[1]


def test_fits_of_mixed_origin(ctx):
    """handles of two fit_batch calls and of one fit() in one list: the call cuts it into runs"""
    n, m = 260, 33
    covs, data = _problems(n, 6, 51, False)
    models, datasets, first = _fit(ctx, covs[:3], data[:3])
    _, _, second = _fit(ctx, covs[3:5], data[3:5])
    lone = ab.gp_from_covariance(covs[5], context=ctx).fit(ab.RegressionDataset(data[5][0], data[5][1]))
    fms = [first[0], second[0], second[1], lone, first[2], first[1]]
    xs = [np.random.default_rng(b).uniform(0., 10., (m, 3)) for b in range(len(fms))]
    for what in WHATS:
        preds = ab.predict_batch(fms, xs, what=what)
        for b, fm in enumerate(fms):
            _check(preds[b], _single(fm, xs[b], what), what, f"mixed origin problem {b} vs predict()")


# ---- the C ABI directly ---------------------------------------------------------------------------------------------

class _Raw:
    """handles of one agp_fit_create_batch call (failed problems included) and everything an agp_predict_batch call needs"""

    def __init__(self, ctx, covs, data, m, seed=5):
        self.ctx, self.count, self.m = ctx, len(covs), m
        n = data[0][0].shape[0]
        self.train = [c.features(x) for c, (x, _, _) in zip(covs, data)]
        self.train_structs = [f.as_struct() for f in self.train]
        self.kernels = [ctx.private_kernel(c) for c in covs]
        Y = np.asfortranarray(np.stack([y for _, y, _ in data], axis=1))
        self.fits = (C.c_void_p * self.count)()
        self.fit_status = (C.c_int * self.count)()
        karr = (C.c_void_p * self.count)(*self.kernels)
        farr = (C.c_void_p * self.count)(*[C.addressof(s) for s in self.train_structs])
        rc = ctx._lib.agp_fit_create_batch(ctx._h, self.count, karr, farr, Y.ctypes.data_as(C.c_void_p), n, None, 0, self.fits, None, 0, None,
                                           self.fit_status)
        assert rc == capi.AGP_OK
        rng = np.random.default_rng(seed)
        self.xs = [rng.uniform(0., 10., (m, 3)) for _ in range(self.count)]
        self.test = [c.features(x) for c, x in zip(covs, self.xs)]
        self.structs = [f.as_struct() for f in self.test]

    def call(self, mode, **over):
        count, m = over.get("count", self.count), self.m
        ldm, lds = over.get("ldm", m), over.get("lds", m if mode == 1 else m * m)
        mean = np.full((max(ldm, m), self.count), 7.0, order="F")
        second = np.full((max(lds, 1), self.count), 7.0, order="F")
        status = (C.c_int * self.count)(*([-5] * self.count))
        karr = over.get("kernels", (C.c_void_p * self.count)(*self.kernels))
        farr = over.get("fits", (C.c_void_p * self.count)(*[self.fits[b] for b in range(self.count)]))
        xarr = over.get("xs", (C.c_void_p * self.count)(*[C.addressof(s) for s in self.structs]))
        rc = self.ctx._lib.agp_predict_batch(self.ctx._h, count, karr, farr, xarr, over.get("mode", mode), mean.ctypes.data_as(C.c_void_p), ldm,
                                             None if over.get("no_second") else second.ctypes.data_as(C.c_void_p), lds,
                                             over.get("out_location", capi.HOST), status)
        return rc, mean, second, list(status)

    def single(self, b, mode):
        mean, second = np.empty(self.m), np.empty(self.m if mode == 1 else self.m * self.m)
        lib, h, k, f, s = self.ctx._lib, self.ctx._h, self.kernels[b], self.fits[b], C.byref(self.structs[b])
        if mode == 0:
            rc = lib.agp_predict_mean(h, k, f, s, mean.ctypes.data_as(C.c_void_p), capi.HOST)
        elif mode == 1:
            rc = lib.agp_predict_marginal(h, k, f, s, mean.ctypes.data_as(C.c_void_p), second.ctypes.data_as(C.c_void_p), capi.HOST)
        else:
            rc = lib.agp_predict_joint(h, k, f, s, mean.ctypes.data_as(C.c_void_p), second.ctypes.data_as(C.c_void_p), capi.HOST)
        assert rc == capi.AGP_OK
        return mean, second

    def close(self):
        for b in range(self.count):
            if self.fits[b]:
                self.ctx._lib.agp_fit_destroy(C.c_void_p(self.fits[b]))
        for k in self.kernels:
            self.ctx._lib.agp_kernel_destroy(k)


@pytest.fixture
def raw_with_failure(ctx):
    n, m = 300, 33
    covs, data = _problems(n, 6, 11, False)
    covs[1] = ab.SquaredExponential(1., 1.)  # no noise + a duplicated point: singular at pivot 5
    data[1][0][5] = data[1][0][2]
    data[5][0][7, 1] = np.nan  # NaN input
    # (problems 2, 3, 4 form a run between the failures: the lock-step path; problem 0 goes alone)
    raw = _Raw(ctx, covs, data, m)
    yield raw
    raw.close()


def test_failed_fits_report_their_status_and_leave_the_neighbours_alone(ctx, raw_with_failure):
    raw = raw_with_failure
    assert list(raw.fit_status) == [capi.AGP_OK, capi.AGP_ERR_NOT_POSITIVE_DEFINITE, capi.AGP_OK, capi.AGP_OK, capi.AGP_OK, capi.AGP_ERR_NAN_INPUT]
    for mode in (0, 1, 2):
        rc, mean, second, status = raw.call(mode)
        assert rc == capi.AGP_OK
        assert status == list(raw.fit_status)
        per = raw.m if mode == 1 else raw.m * raw.m
        for b in range(raw.count):
            if status[b] != capi.AGP_OK:
                assert np.isnan(mean[:raw.m, b]).all()
                assert mode == 0 or np.isnan(second[:per, b]).all()
                continue
            sm, ss = raw.single(b, mode)
            _close(mean[:raw.m, b], sm, 0., f"mode {mode} problem {b} mean vs single")
            if mode:
                _close(second[:per, b], ss, 1e-9, f"mode {mode} problem {b} second moment vs single")


def test_malformed_arguments_write_nothing(ctx, raw_with_failure):
    raw = raw_with_failure
    m, count = raw.m, raw.count

    def rejected(mode=1, **over):
        rc, mean, second, status = raw.call(mode, **over)
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT, over
        assert (mean == 7.0).all() and (second == 7.0).all() and status == [-5] * count, over

    rejected(count=0)
    rejected(count=-1)
    rejected(mode=3)
    rejected(mode=-1)
    rejected(ldm=m - 1)
    rejected(mode=1, lds=m - 1)
    rejected(mode=2, lds=m * m - 1)
    rejected(no_second=True)
    rejected(out_location=2)
    for name, arr in (("kernels", raw.kernels), ("fits", [raw.fits[b] for b in range(count)]), ("xs", [C.addressof(s) for s in raw.structs])):
        holed = list(arr)
        holed[2] = None
        rejected(**{name: (C.c_void_p * count)(*holed)})
    # unequal m, mixed locations, a dimension mismatch
    for field, value in (("n", m - 1), ("location", capi.DEVICE), ("dim", 2)):
        keep = getattr(raw.structs[2], field)
        setattr(raw.structs[2], field, value)
        try:
            rejected()
        finally:
            setattr(raw.structs[2], field, keep)
    # unequal n: a fit of another size; a fit without training features (agp_factor_create)
    other_covs, other_data = _problems(200, 1, 3, False)
    other = _Raw(ctx, other_covs, other_data, m)
    K = np.asfortranarray(np.eye(300) * 2.0)
    factor = C.c_void_p()
    assert ctx._lib.agp_factor_create(ctx._h, K.ctypes.data_as(C.c_void_p), 300, 300, 0, capi.HOST, C.byref(factor)) == capi.AGP_OK
    try:
        for intruder in (other.fits[0], factor.value):
            fits = [raw.fits[b] for b in range(count)]
            fits[4] = intruder
            rejected(fits=(C.c_void_p * count)(*fits))
    finally:
        other.close()
        ctx._lib.agp_fit_destroy(factor)


def test_zero_test_points_is_ok(ctx, raw_with_failure):
    raw = raw_with_failure
    keep = [s.n for s in raw.structs]
    for s in raw.structs:
        s.n = 0
    try:
        saved, raw.m = raw.m, 0
        rc, mean, second, status = raw.call(1, ldm=1, lds=1)
        raw.m = saved
        assert rc == capi.AGP_OK and (mean == 7.0).all() and (second == 7.0).all()
    finally:
        for s, n in zip(raw.structs, keep):
            s.n = n


def test_device_outputs_hold_the_same_numbers(ctx, raw_with_failure):
    raw = raw_with_failure
    m, count = raw.m, raw.count
    for mode in (0, 1, 2):
        per = m if mode == 1 else m * m
        rc, mean, second, status = raw.call(mode)
        assert rc == capi.AGP_OK
        ldm, lds = m + 3, per + 5  # padded leading dimensions: the padding stays untouched
        dmean, dsecond = ctx.to_device(np.full(ldm * count, 7.0)), ctx.to_device(np.full(lds * count, 7.0))
        dstatus = (C.c_int * count)()
        karr = (C.c_void_p * count)(*raw.kernels)
        farr = (C.c_void_p * count)(*[raw.fits[b] for b in range(count)])
        xarr = (C.c_void_p * count)(*[C.addressof(s) for s in raw.structs])
        assert ctx._lib.agp_predict_batch(ctx._h, count, karr, farr, xarr, mode, C.c_void_p(dmean.ptr), ldm, C.c_void_p(dsecond.ptr), lds,
                                          capi.DEVICE, dstatus) == capi.AGP_OK
        assert list(dstatus) == status
        got_mean = dmean.numpy().reshape((ldm, count), order="F")
        got_second = dsecond.numpy().reshape((lds, count), order="F")
        assert np.array_equal(got_mean[:m], mean[:m], equal_nan=True) and (got_mean[m:] == 7.0).all()
        if mode:
            assert np.array_equal(got_second[:per], second[:per], equal_nan=True) and (got_second[per:] == 7.0).all()
        else:
            assert (got_second == 7.0).all()
