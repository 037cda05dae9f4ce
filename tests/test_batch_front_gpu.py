"""The three batched fits that share one front end (csrc/batch_front.h) pinned to each other: agp_nll_batch,
agp_fit_create_batch and agp_nll_gradient_batch (with agp_loo_nll_gradient_batch for the argument check) build the same
Gram slabs and factor them in lock step, so one problem's negative log likelihood must come out the same from all three:

  - agp_nll_gradient_batch with n_slots = 0: its value;
  - agp_fit_create_batch: 0.5 (log_det + y . information + n log 2 pi), rebuilt on the host;
  - agp_nll_batch (no target variance, or one variance vector shared by all problems): its value.

Tolerance between any two: 1e-9 max(1, |nll|), what test_gp_gpu.py uses between a batched and a single evaluation.
agp_nll_batch and agp_nll_gradient_batch make the same launches at these sizes (no look-ahead) and finish with the same
host expression: they were bit-equal before the front end was shared (every case below, measured on the parent commit) and
are asserted bit-equal here.

Sizes: n = 100 inside one 128-row block, 129 one row past it, 520 past one 512-row outer block; count 1 (the per-problem
Gram launch) and 3; uniform trees (one Gram launch for the batch, one feature array shared by all problems) and mixed
trees (a Gram launch each, features of their own); one target vector shared by all (ld = 0) and one per problem."""
import ctypes as C
import itertools

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi

pytestmark = pytest.mark.gpu

MARK = 7.0


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _cov(kind, b):
    f = 1. + 0.1 * b
    which = 0 if kind == "uniform" else (b + 1) % 3
    if which == 0:
        return ab.SquaredExponential(1.2 * f, 1.0 / f) + ab.IndependentNoise(0.1 * f)
    if which == 1:
        return ab.Matern52(2.0 * f, 0.8) + ab.IndependentNoise(0.15)
    return ab.Matern32(2.0, 1.0 * f) * ab.Constant(0.6) + ab.IndependentNoise(0.12)


class _Batch:
    """`count` problems of n points and the calls of the three entries on them, every array kept alive"""

    def __init__(self, ctx, n, count, kind, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.n, self.count = ctx, n, count
        self.covs = [_cov(kind, b) for b in range(count)]
        shared = rng.uniform(0., 10., (n, 3))
        self.xs = [shared if kind == "uniform" else rng.uniform(0., 10., (n, 3)) for _ in range(count)]
        self.Y = np.asfortranarray(np.stack([np.sin(x).sum(axis=1) + 0.1 * b for b, x in enumerate(self.xs)], axis=1))
        self.V = np.asfortranarray(rng.uniform(0.01, 0.1, (n, count)))

    def _arguments(self):
        fsets, cache = [], {}
        for cov, x in zip(self.covs, self.xs):  # problems on one array share one FeatureSet: the same pointers
            if id(x) not in cache:
                cache[id(x)] = cov.features(x)
            fsets.append(cache[id(x)])
        structs = [fs.as_struct() for fs in fsets]
        handles = [self.ctx.private_kernel(cov) for cov in self.covs]
        return fsets, structs, handles

    def nlls(self, shared_y, var):
        """(agp_nll_gradient_batch, host rebuild from agp_fit_create_batch, agp_nll_batch or None), each with its
        per-problem status (None for agp_nll_batch).  var: None | "shared" | "each"."""
        ctx, n, count = self.ctx, self.n, self.count
        lib = ctx._lib
        fsets, structs, handles = self._arguments()
        try:
            kernels = (C.c_void_p * count)(*handles)
            fptrs = (C.c_void_p * count)(*[C.addressof(s) for s in structs])
            ldy, ldv = (0 if shared_y else n), (0 if var == "shared" else n)
            v_ptr = None if var is None else _p(self.V)
            # agp_nll_gradient_batch, value only
            g_val = np.full(count, MARK)
            g_status = (C.c_int * count)(*([-5] * count))
            zeros = (C.c_int * count)()
            rc = lib.agp_nll_gradient_batch(ctx._h, count, kernels, fptrs, _p(self.Y), ldy, v_ptr, ldv, zeros, None, None, 0, _p(g_val), None, 0,
                                            None, 0, g_status)
            assert rc == capi.AGP_OK
            # agp_fit_create_batch
            fits = (C.c_void_p * count)()
            f_status = (C.c_int * count)(*([-5] * count))
            info = np.full((count, n), MARK)
            log_det = np.full(count, MARK)
            rc = lib.agp_fit_create_batch(ctx._h, count, kernels, fptrs, _p(self.Y), ldy, v_ptr, ldv, fits, _p(info), n, _p(log_det), f_status)
            assert rc == capi.AGP_OK
            for f in fits:
                lib.agp_fit_destroy(C.c_void_p(f))
            f_val = np.array([0.5 * (log_det[b] + self.Y[:, 0 if shared_y else b] @ info[b] + n * np.log(2. * np.pi)) if f_status[b] == 0
                              else np.nan for b in range(count)])
            # agp_nll_batch: one variance vector for all problems or none
            b_val = None
            if var != "each":
                b_val = np.full(count, MARK)
                rc = lib.agp_nll_batch(ctx._h, count, kernels, fptrs, _p(self.Y), ldy, v_ptr, _p(b_val))
                assert rc == capi.AGP_OK
        finally:
            for h in handles:
                lib.agp_kernel_destroy(h)
        return (g_val, list(g_status)), (f_val, list(f_status)), (b_val, None)


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("n", [100, 129, 520])
def test_three_entries_agree_on_the_likelihood(ctx, n, count):
    for kind, shared_y, var in itertools.product(("uniform", "mixed"), (True, False), (None, "shared", "each")):
        case = (n, count, kind, shared_y, var)
        batch = _Batch(ctx, n, count, kind, 1000 * n + count)
        (g_val, g_status), (f_val, f_status), (b_val, _) = batch.nlls(shared_y, var)
        assert g_status == [0] * count and f_status == [0] * count, case
        for b in range(count):
            tol = 1e-9 * max(1., abs(g_val[b]))
            print(case, b, "gradient", g_val[b], "fit - gradient", f_val[b] - g_val[b],
                  "nll_batch - gradient", None if b_val is None else b_val[b] - g_val[b])
            assert abs(f_val[b] - g_val[b]) <= tol, (case, b)
            if b_val is not None:
                assert abs(b_val[b] - f_val[b]) <= tol, (case, b)
        if b_val is not None:
            assert b_val.tobytes() == g_val.tobytes(), case


@pytest.mark.parametrize("n", [100, 129, 520])
def test_a_failed_problem_is_reported_in_its_slot_by_all_three(ctx, n):
    """count = 3, problem 1 without noise on a duplicated point: NaN from agp_nll_batch, AGP_ERR_NOT_POSITIVE_DEFINITE from
    the other two, and problems 0 and 2 bit for bit what they are in a batch without the failure"""
    good = _Batch(ctx, n, 3, "mixed", n)
    bad = _Batch(ctx, n, 3, "mixed", n)
    bad.covs[1] = ab.SquaredExponential(1., 1.)
    bad.xs[1] = bad.xs[1].copy()
    bad.xs[1][5] = bad.xs[1][0]  # K_00 = K_05 = K_55 exactly: a zero pivot
    want = good.nlls(False, None)
    got = bad.nlls(False, None)
    (g_val, g_status), (f_val, f_status), (b_val, _) = got
    npd = capi.AGP_ERR_NOT_POSITIVE_DEFINITE
    assert g_status == [0, npd, 0] and f_status == [0, npd, 0]
    assert np.isnan(g_val[1]) and np.isnan(f_val[1]) and np.isnan(b_val[1])
    for (w, _), (v, _) in zip(want, got):
        assert not np.isnan(v[[0, 2]]).any()
        assert v[[0, 2]].tobytes() == w[[0, 2]].tobytes()


def test_more_problems_than_a_grid_dimension_holds_are_refused(ctx):
    """count = 65536 (gridDim.y of the batched launches ends at 65535): AGP_ERR_INVALID_ARGUMENT from all four entries,
    nothing written.  Every pointer aliases one small problem, so nothing is allocated for the batch."""
    count, n = 65536, 4
    lib = ctx._lib
    cov = ab.SquaredExponential(1., 1.) + ab.IndependentNoise(0.1)
    fs = cov.features(np.random.default_rng(0).uniform(0., 10., (n, 3)))
    struct = fs.as_struct()
    y = np.arange(1., n + 1.)
    handle = ctx.private_kernel(cov)
    try:
        kernels = (C.c_void_p * count)(*([handle.value] * count))
        fptrs = (C.c_void_p * count)(*([C.addressof(struct)] * count))
        value = np.full(count, MARK)
        assert lib.agp_nll_batch(ctx._h, count, kernels, fptrs, _p(y), 0, None, _p(value)) == capi.AGP_ERR_INVALID_ARGUMENT
        assert (value == MARK).all()
        fits = (C.c_void_p * count)(*([0xBAD] * count))
        status = (C.c_int * count)(*([-5] * count))
        info = np.full((count, n), MARK)
        log_det = np.full(count, MARK)
        rc = lib.agp_fit_create_batch(ctx._h, count, kernels, fptrs, _p(y), 0, None, 0, fits, _p(info), n, _p(log_det), status)
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT
        assert all(f == 0xBAD for f in fits) and all(s == -5 for s in status) and (info == MARK).all() and (log_det == MARK).all()
        zeros = (C.c_int * count)()
        for entry in (lib.agp_nll_gradient_batch, lib.agp_loo_nll_gradient_batch):
            grad = np.full((count, 1), MARK)
            vec = np.full((count, n), MARK)
            rc = entry(ctx._h, count, kernels, fptrs, _p(y), 0, None, 0, zeros, None, None, 0, _p(value), _p(grad), 1, _p(vec), n, status)
            assert rc == capi.AGP_ERR_INVALID_ARGUMENT
            assert (value == MARK).all() and (grad == MARK).all() and (vec == MARK).all() and all(s == -5 for s in status)
    finally:
        lib.agp_kernel_destroy(handle)
