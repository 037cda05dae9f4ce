"""agp_fit_create_batch_ragged, and agp_predict_batch / agp_fit_update_batch on fits of unequal real sizes (include/
albatross_amd.h; csrc/ragged_batch.hip), with ab.fit_batch / predict_batch / update_batch over size classes: against the
oracle and the per-model fit / predict / update, at the edges of the 128-row block (a second panel made of phantom rows
only, a problem whose phantom range is exactly that panel, one without phantoms, one of a single point), past the 512-row
outer block, with generic trees, scale columns and equality ids, failed problems and malformed arguments.

Bounds: the ones the project holds equal-size batches to - information 1e-8 max|ref| and log determinant 1e-6 n against the
oracle, 1e-9 against fit() (tests/test_fit_batch_gpu.py); predictions mean 1e-8 max|ref|, second moment 1e-8 max|ref| +
1e-9; L L^T 1e-10 max|K|; updates 1e-8 against the oracle and 2e-8 against update() (tests/test_update_batch_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from oracle import oracle_py as orc
import update_batch_cases as ubc

pytestmark = pytest.mark.gpu

WHATS = ("mean", "marginal", "joint")


def _close(got, ref, relative, absolute, what):
    err, bound = np.abs(np.asarray(got) - np.asarray(ref)).max(), relative * np.abs(ref).max() + absolute
    print(f"{what}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


def _problems(sizes, seed, tree="mixed", with_variance=True, dim=3):
    """one ubc.Problem per size.  tree "mixed": two operators in the batch (a Gram launch per problem), "uniform": one
    radial + noise tree (the one-launch Gram), or a kind of update_batch_cases.  with_variance: target variances on the
    even problems, and a duplicated point there where n_b >= 6 (the variance keeps K definite)"""
    rng = np.random.default_rng(seed)
    out = []
    for b, n in enumerate(sizes):
        mean = None
        if tree == "mixed":
            cov = (ab.Matern52(1.5 + 0.25 * b, 1.0) if b % 3 else ab.SquaredExponential(1.0 + 0.1 * b, 1.2)) + ab.IndependentNoise(0.1 + 0.01 * b)
        elif tree == "uniform":
            cov = ab.Matern52(1.5 + 0.02 * b, 1.0) + ab.IndependentNoise(0.1 + 0.002 * b)
        else:
            cov, mean, dim = ubc.covariance(tree, b)
        x = rng.uniform(0., 10., (n, dim))
        var = rng.uniform(0.01, 0.05, n) if with_variance and b % 2 == 0 else None
        if var is not None and n >= 6:
            x[5] = x[2]
        y = np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) + 0.05 * b
        out.append(ubc.Problem(cov, mean, x, y, var))
    return out


ALL = slice(None)


def _matrix(p):
    return orc.gram(p.cov, p.x, x_meas=True) + (0. if p.var is None else np.diag(p.var))


class RaggedCall:
    """one agp_fit_create_batch_ragged (or agp_fit_create_batch) call at the C-ABI level, inputs in host memory or resident in
    HBM.  Past its n_b values
    a column of y / y_var holds NaN (never read), a column of `information` the sentinel -7 (never written)."""

    def __init__(self, ctx, probs, entry="agp_fit_create_batch_ragged", where="host"):
        self.ctx, self.probs, self.count, self.entry = ctx, probs, len(probs), entry
        self.models = [p.model(ctx) for p in probs]
        self.fsets = [m.covariance_function_.features(p.x) for m, p in zip(self.models, probs)]
        self.sizes = [fs.n for fs in self.fsets]
        self.n = max(self.sizes)
        self.Y = np.full((self.n, self.count), np.nan, order="F")
        self.have_var = any(p.var is not None for p in probs)
        self.V = np.full((self.n, self.count), np.nan, order="F")
        for b, (m, fs, p) in enumerate(zip(self.models, self.fsets, probs)):
            y, v = m._targets(fs, p.dataset(ALL).targets)
            self.Y[:fs.n, b] = y
            self.V[:fs.n, b] = 0. if v is None else v
        self.structs = [fs.as_struct() for fs in self.fsets]
        self.y_ptr, self.v_ptr, self.keep = abgp._ptr(self.Y), abgp._ptr(self.V), []
        if where == "device":
            for fs, s in zip(self.fsets, self.structs):
                for field, a in (("coords", fs.coords), ("eq_id", fs.eq_id), ("scales", fs.scales)):
                    if a is not None:
                        self.keep.append(ubc._to_device(ctx, a))
                        setattr(s, field, self.keep[-1].ptr)
                s.location = capi.DEVICE
            self.keep += [ubc._to_device(ctx, self.Y), ubc._to_device(ctx, self.V)]
            self.y_ptr, self.v_ptr = C.c_void_p(self.keep[-2].ptr), C.c_void_p(self.keep[-1].ptr)
        self.kernels = [ctx.private_kernel(m.covariance_function_) for m in self.models]
        self.information = np.full((self.n + 3, self.count), -7.0, order="F")
        self.log_det = np.full(self.count, -7.0)
        self.status = (C.c_int * self.count)(*([-99] * self.count))
        self.out = (C.c_void_p * self.count)(*([0xdead] * self.count))

    def run(self, count=None, ldy=None, ldi=None, kernels=None, structs=None):
        count = self.count if count is None else count
        kernels = self.kernels if kernels is None else kernels
        fptrs = [C.addressof(s) for s in self.structs] if structs is None else structs
        return getattr(self.ctx._lib, self.entry)(
            self.ctx._h, count, (C.c_void_p * self.count)(*kernels), (C.c_void_p * self.count)(*fptrs), self.y_ptr,
            self.n if ldy is None else ldy, self.v_ptr if self.have_var else None, self.n, self.out, abgp._ptr(self.information),
            self.n + 3 if ldi is None else ldi, abgp._ptr(self.log_det), self.status)

    def untouched(self):
        return (list(self.status) == [-99] * self.count and [self.out[b] for b in range(self.count)] == [0xdead] * self.count
                and np.all(self.information == -7.0) and np.all(self.log_det == -7.0))

    def fits(self):
        """the published handles as GPFits (which destroy them)"""
        return [abgp.GPFit(self.ctx, C.c_void_p(self.out[b]), self.sizes[b], self.probs[b].x) for b in range(self.count)]

    def close(self):
        for k in self.kernels:
            self.ctx._lib.agp_kernel_destroy(k)
        self.kernels = []


def _check_fit(ctx, call, b, fit, xs):
    """problem b of a call against the oracle and against model.fit"""
    p, n = call.probs[b], call.sizes[b]
    label = f"n_b={n} problem {b}"
    of = p.oracle(ALL)
    assert ctx._lib.agp_fit_size(fit._h) == n and ctx._lib.agp_fit_padded_size(fit._h) == call.n
    assert ctx._lib.agp_fit_failed_pivot(fit._h) == -1
    _close(call.information[:n, b], of.information, 1e-8, 0., f"{label} information vs oracle")
    assert np.all(call.information[n:, b] == -7.0), f"{label}: the information column was written past n_b"
    assert np.array_equal(fit.information, call.information[:n, b])
    K = _matrix(p)
    err = abs(call.log_det[b] - np.linalg.slogdet(K)[1])
    print(f"{label} log determinant: error {err:.3e}, bound {1e-6 * n:.3e}")
    assert err <= 1e-6 * n and fit.log_determinant == call.log_det[b]
    L = fit.factor()
    assert L.shape == (n, n)
    _close(L @ L.T, K, 1e-10, 0., f"{label} L L^T")
    rhs = np.random.default_rng(b).standard_normal((n, 2))
    _close(fit.solve(rhs), of.solve(rhs), 1e-8, 0., f"{label} solve")
    fm = abgp.FitModel(call.models[b], fit)
    om, ov = of.predict_marginal(xs)
    marg = fm.predict(xs).marginal()
    _close(marg.mean, om, 1e-8, 0., f"{label} marginal mean")
    _close(marg.covariance, ov, 1e-8, 1e-9, f"{label} marginal variance")
    single = call.models[b].fit(p.dataset(ALL)).get_fit()
    _close(fit.information, single.information, 1e-9, 0., f"{label} information vs fit()")
    assert abs(fit.log_determinant - single.log_determinant) <= 1e-9 * max(n, 1) + 1e-12


def _run_and_check(ctx, probs, dim=3):
    call = RaggedCall(ctx, probs)
    try:
        assert call.run() == capi.AGP_OK
        assert list(call.status) == [capi.AGP_OK] * call.count
        fits = call.fits()
        xs = np.random.default_rng(3).uniform(0., 10., (33, dim))
        for b, fit in enumerate(fits):
            _check_fit(ctx, call, b, fit, xs)
        del fits[1]  # any order
        del fits
    finally:
        call.close()


def test_c_entry_at_the_block_edges(ctx):
    """padded size 130: a two-row second panel made of phantom rows only (129 has one real row in it), a problem whose
    phantom range is exactly that panel (128), one without phantom rows (130), one of a single point"""
    _run_and_check(ctx, _problems([1, 2, 31, 33, 127, 128, 129, 130], 7, "mixed"))


def test_one_launch_gram_past_the_outer_block(ctx):
    _run_and_check(ctx, _problems([200, 256, 257, 385, 512, 513, 640], 11, "uniform"))


@pytest.mark.parametrize("kind", ["dim4", "scaling", "update_tree"])
def test_generic_trees_scale_columns_and_equality_ids(ctx, kind):
    probs = _problems([100, 130, 131], 13, kind)
    _run_and_check(ctx, probs, probs[0].x.shape[1])


def test_equal_sizes_give_the_bits_of_the_equal_size_entry(ctx):
    probs = _problems([300] * 4, 17, "mixed")
    results = []
    for entry in ("agp_fit_create_batch", "agp_fit_create_batch_ragged"):
        call = RaggedCall(ctx, probs, entry)
        try:
            assert call.run() == capi.AGP_OK
            fits = call.fits()
            assert all(ctx._lib.agp_fit_padded_size(f._h) == 300 for f in fits)
            results.append((call.information.copy(), call.log_det.copy(), [f.factor() for f in fits]))
            del fits
        finally:
            call.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    for a, b in zip(results[0][2], results[1][2]):
        assert np.array_equal(a, b)


def test_failed_problems_fail_alone(ctx):
    probs = _problems([90, 200, 131, 256, 140], 19, "mixed", with_variance=False)
    probs[1].cov = ab.SquaredExponential(1., 1.)  # no noise + a duplicated point: singular at pivot 5
    probs[1].x[5] = probs[1].x[2]
    probs[3].x[7, 1] = np.nan
    call = RaggedCall(ctx, probs)
    try:
        assert call.run() == capi.AGP_OK
        assert list(call.status) == [capi.AGP_OK, capi.AGP_ERR_NOT_POSITIVE_DEFINITE, capi.AGP_OK, capi.AGP_ERR_NAN_INPUT, capi.AGP_OK]
        fits = call.fits()
        assert ctx._lib.agp_fit_failed_pivot(fits[1]._h) == 5
        assert np.all(call.information[:, 1] == -7.0) and np.all(call.information[:, 3] == -7.0)
        for b in (0, 2, 4):
            _close(call.information[:call.sizes[b], b], probs[b].oracle(ALL).information, 1e-8, 0., f"neighbour {b} of the failures")
        del fits
    finally:
        call.close()
    models = [p.model(ctx) for p in probs]
    with pytest.raises(ab.NotPositiveDefiniteError, match="problem 1 .pivot 5."):
        ab.fit_batch(models, [p.dataset(ALL) for p in probs])
    probs[1].cov = ab.SquaredExponential(1., 1.) + ab.IndependentNoise(0.1)
    models = [p.model(ctx) for p in probs]
    with pytest.raises(ab.NanInputError, match="problem 3"):
        ab.fit_batch(models, [p.dataset(ALL) for p in probs])


def test_malformed_arguments_write_nothing(ctx):
    probs = _problems([100, 130, 64], 23, "uniform")
    call = RaggedCall(ctx, probs)
    dev = ctx.to_device(np.ascontiguousarray(probs[1].x))
    try:
        empty = call.fsets[2].as_struct()
        empty.n = 0
        moved = call.fsets[1].as_struct()
        moved.coords, moved.location = dev.ptr, capi.DEVICE
        ptrs = [C.addressof(s) for s in call.structs]
        cases = [{"ldy": 129}, {"ldi": 129}, {"count": 0}, {"count": 65536},
                 {"structs": ptrs[:2] + [C.addressof(empty)]}, {"structs": [ptrs[0], C.addressof(moved), ptrs[2]]},
                 {"structs": [ptrs[0], None, ptrs[2]]}, {"kernels": [call.kernels[0], None, call.kernels[2]]}]
        for kwargs in cases:
            assert call.run(**kwargs) == capi.AGP_ERR_INVALID_ARGUMENT, kwargs
            assert call.untouched(), kwargs
        assert call.run() == capi.AGP_OK  # the same arguments, well formed
        del_fits = call.fits()
        del del_fits
    finally:
        call.close()


def test_two_identical_calls_give_the_same_bits(ctx):
    probs = _problems([97, 129, 255, 256, 200], 29, "mixed")
    results = []
    for _ in range(2):
        call = RaggedCall(ctx, probs)
        try:
            assert call.run() == capi.AGP_OK
            fits = call.fits()
            results.append((call.information.copy(), call.log_det.copy(), [f.factor() for f in fits]))
            del fits
        finally:
            call.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    for a, b in zip(results[0][2], results[1][2]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", ["uniform", "scaling", "update_tree"])
def test_device_resident_inputs_give_the_bits_of_host_inputs(ctx, kind):
    """features, targets and variances in HBM go through the table-driven copy launch (scale columns to the stride of the
    padded features, n_b values of every target column)"""
    probs = _problems([100, 130, 131, 64], 59, kind)
    results = []
    for where in ("host", "device"):
        call = RaggedCall(ctx, probs, where=where)
        try:
            assert call.run() == capi.AGP_OK and list(call.status) == [capi.AGP_OK] * call.count
            fits = call.fits()
            results.append((call.information.copy(), call.log_det.copy(), [f.factor() for f in fits]))
            del fits
        finally:
            call.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    for a, b in zip(results[0][2], results[1][2]):
        assert np.array_equal(a, b)
    _close(results[1][0][:131, 2], probs[2].oracle(ALL).information, 1e-8, 0., "device inputs, information vs oracle")


def _check_pred(pred, ref, what, label):
    if what == "mean":
        _close(pred, ref[0], 1e-8, 0., f"{label} mean")
    else:
        _close(pred.mean, ref[0], 1e-8, 0., f"{label} {what} mean")
        _close(pred.covariance, ref[1], 1e-8, 1e-9, f"{label} {what} second moment")


def _oracle_pred(of, xs, what, xs_meas=False):
    if what == "mean":
        return (of.predict_mean(xs, xs_meas),)
    return of.predict_marginal(xs, xs_meas) if what == "marginal" else of.predict_joint(xs, xs_meas)


def _single_pred(fm, xs, what):
    p = fm.predict(xs)
    if what == "mean":
        return (p.mean(),)
    d = p.marginal() if what == "marginal" else p.joint()
    return d.mean, d.covariance


@pytest.mark.parametrize("sizes,tree", [([100, 127, 128], "mixed"), ([100, 127, 128], "uniform"),
                                        ([129, 200, 256, 300, 384], "uniform"), ([129, 200, 256, 300, 384], "mixed")])
def test_predict_batch_on_ragged_fits(ctx, sizes, tree):
    probs = _problems(sizes, 31 + len(sizes), tree)
    models = [p.model(ctx) for p in probs]
    fms = ab.fit_batch(models, [p.dataset(ALL) for p in probs])
    ofs = [p.oracle(ALL) for p in probs]
    rng = np.random.default_rng(3)
    for m in (1, 33, 64, 65):
        xs = [rng.uniform(0., 10., (m, 3)) for _ in probs]
        for what in WHATS:
            preds = ab.predict_batch(fms, xs, what=what)
            for b in range(len(probs)):
                _check_pred(preds[b], _oracle_pred(ofs[b], xs[b], what), what, f"{tree} n_b={sizes[b]} m={m} vs oracle")
                _check_pred(preds[b], _single_pred(fms[b], xs[b], what), what, f"{tree} n_b={sizes[b]} m={m} vs predict()")
            if what == "joint":
                for p in preds:
                    assert np.array_equal(p.covariance, p.covariance.T)  # mirrored bit for bit


def test_phantom_rows_add_no_noise_covariance(ctx):
    """Measurement-wrapped test points that include each problem's FIRST training point: the phantom rows hold copies of
    it, so an unzeroed phantom row of the cross covariance would add noise covariance there.  The mean-only kernel reads
    the phantom rows too and relies on the information vector being zero there."""
    sizes = [100, 127, 128, 90]
    probs = _problems(sizes, 37, "uniform", with_variance=False)
    models = [p.model(ctx) for p in probs]
    fms = ab.fit_batch(models, [p.dataset(ALL) for p in probs])
    rng = np.random.default_rng(5)
    xs = [np.concatenate([p.x[:3], rng.uniform(0., 10., (30, 3))]) for p in probs]
    for what in WHATS:
        preds = ab.predict_batch(fms, [ab.Measurement(x) for x in xs], what=what)
        for b, p in enumerate(probs):
            _check_pred(preds[b], _oracle_pred(p.oracle(ALL), xs[b], what, xs_meas=True), what, f"first training point, n_b={sizes[b]}")


def test_predict_batch_mixes_ragged_and_grown_fits(ctx):
    """fits grown by update_batch from 250 points (phantom range [250, 256) in the middle) beside ragged fits (trailing
    phantom range) of the same padded size 300"""
    grown_probs = _problems([294, 294], 41, "uniform")
    gm = [p.model(ctx) for p in grown_probs]
    old = ab.fit_batch(gm, [p.dataset(slice(0, 250)) for p in grown_probs])
    grown = ab.update_batch(old, [p.dataset(slice(250, 294)) for p in grown_probs])
    ragged_probs = _problems([280, 300, 258], 43, "uniform")
    fms = ab.fit_batch([p.model(ctx) for p in ragged_probs], [p.dataset(ALL) for p in ragged_probs])
    every = fms[:2] + grown + fms[2:]
    assert {ctx._lib.agp_fit_padded_size(fm.get_fit()._h) for fm in every} == {300}
    xs = np.random.default_rng(6).uniform(0., 10., (33, 3))
    for what in WHATS:
        preds = ab.predict_batch(every, xs, what=what)
        for b, fm in enumerate(every):
            _check_pred(preds[b], _single_pred(fm, xs, what), what, f"mixed origin problem {b} vs predict()")
    # the handles of the two calls interleaved: the results still come back in the caller's order
    shuffled = [fms[0], grown[1], fms[2], grown[0], fms[1]]
    for what in WHATS:
        preds = ab.predict_batch(shuffled, xs, what=what)
        for b, fm in enumerate(shuffled):
            _check_pred(preds[b], _single_pred(fm, xs, what), what, f"interleaved problem {b} vs predict()")
    ofs = [p.oracle_update(p.oracle(slice(0, 250)), slice(250, 294)) for p in grown_probs]
    preds = ab.predict_batch(every, xs, what="marginal")
    for b, of in enumerate(ofs):
        _check_pred(preds[2 + b], of.predict_marginal(xs), "marginal", f"grown problem {b} vs oracle")


@pytest.mark.parametrize("m", [1, 127, 129])
def test_update_batch_on_ragged_fits(ctx, m):
    sizes = [130, 200, 250, 256]
    probs = _problems([n + m + 20 for n in sizes], 47 + m, "uniform")
    models = [p.model(ctx) for p in probs]
    fms = ab.fit_batch(models, [p.dataset(slice(0, n)) for p, n in zip(probs, sizes)])
    assert {ctx._lib.agp_fit_padded_size(fm.get_fit()._h) for fm in fms} == {256}
    news = [slice(n, n + m) for n in sizes]
    grown = ab.update_batch(fms, [p.dataset(sl) for p, sl in zip(probs, news)])
    xs = np.random.default_rng(8).uniform(0., 10., (33, 3))
    ofs = []
    for b, (p, n, sl) in enumerate(zip(probs, sizes, news)):
        fit = grown[b].get_fit()
        assert fit.rows() == n + m and ctx._lib.agp_fit_size(fit._h) == n + m
        assert np.array_equal(fit.train_features, p.x[:n + m])
        of = p.oracle_update(p.oracle(slice(0, n)), sl)
        ofs.append(of)
        _close(fit.information, of.information, 1e-8, 0., f"m={m} n_b={n} information vs oracle")
        single = fms[b].update(p.dataset(sl))
        _close(fit.information, single.get_fit().information, 2e-8, 0., f"m={m} n_b={n} information vs update()")
        assert abs(fit.log_determinant - single.get_fit().log_determinant) <= 2e-8 * (n + m)
        om, ov = of.predict_marginal(xs)
        marg = grown[b].predict(xs).marginal()
        _close(marg.mean, om, 1e-8, 0., f"m={m} n_b={n} mean vs oracle")
        _close(marg.covariance, ov, 1e-8, 1e-10, f"m={m} n_b={n} variance vs oracle")
        sm = single.predict(xs).marginal()
        _close(marg.mean, sm.mean, 2e-8, 0., f"m={m} n_b={n} mean vs update()")
        _close(marg.covariance, sm.covariance, 2e-8, 1e-10, f"m={m} n_b={n} variance vs update()")
    # once more on the grown fits (two phantom ranges each where 256 + m is no multiple of 128), then predict_batch
    again = [slice(n + m, n + m + 20) for n in sizes]
    twice = ab.update_batch(grown, [p.dataset(sl) for p, sl in zip(probs, again)])
    ofs = [p.oracle_update(of, sl) for p, of, sl in zip(probs, ofs, again)]
    for what in WHATS:
        preds = ab.predict_batch(twice, xs, what=what)
        for b, of in enumerate(ofs):
            assert twice[b].get_fit().rows() == sizes[b] + m + 20
            _check_pred(preds[b], _oracle_pred(of, xs, what), what, f"m={m} n_b={sizes[b]} twice updated, {what}")


def test_surfaces_across_size_classes(ctx):
    sizes = [60, 128, 129, 250, 256, 300, 700]
    m = 40
    probs = _problems([n + m for n in sizes], 53, "mixed")
    models = [p.model(ctx) for p in probs]
    fms = ab.fit_batch(models, [p.dataset(slice(0, n)) for p, n in zip(probs, sizes)])
    assert [fm.get_fit().rows() for fm in fms] == sizes
    assert [ctx._lib.agp_fit_padded_size(fm.get_fit()._h) for fm in fms] == [128, 128, 256, 256, 256, 300, 700]
    xs = [np.random.default_rng(b).uniform(0., 10., (33, 3)) for b in range(len(sizes))]
    for b, (p, n) in enumerate(zip(probs, sizes)):
        of = p.oracle(slice(0, n))
        assert fms[b].get_fit().information.shape == (n,)
        _close(fms[b].get_fit().information, of.information, 1e-8, 0., f"fit_batch problem {b} (n_b={n})")
    for what in WHATS:
        preds = ab.predict_batch(fms, xs, what=what)
        for b, (p, n) in enumerate(zip(probs, sizes)):
            _check_pred(preds[b], _oracle_pred(p.oracle(slice(0, n)), xs[b], what), what, f"predict_batch problem {b} (n_b={n})")
    grown = ab.update_batch(fms, [p.dataset(slice(n, n + m)) for p, n in zip(probs, sizes)])
    for b, (p, n) in enumerate(zip(probs, sizes)):
        of = p.oracle_update(p.oracle(slice(0, n)), slice(n, n + m))
        assert grown[b].get_fit().rows() == n + m
        _close(grown[b].get_fit().information, of.information, 1e-8, 0., f"update_batch problem {b} (n_b={n})")
    ref = grown[6].predict(xs[6]).mean()
    for b in (3, 0, 5, 1):  # handles destroyed in any order, old and grown
        fms[b] = None
        grown[b] = None
    _close(grown[6].predict(xs[6]).mean(), ref, 0., 0., "after destroying neighbours")
    del fms, grown
