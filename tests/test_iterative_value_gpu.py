"""The log-likelihood value of the matrix-free fit on the device: pcg_record_kernel and pcg_probe_kernel on their own
(csrc/iterative.hip through the probes of csrc/debug_api.hip), agp_iterative_nll, and IterativeFitModel.log_likelihood /
log_likelihood_and_gradient / get_fit().log_determinant.

The shapes, the seeds, the numpy restatement and every bar are tests/lanczos_value_cases.py's
(tests/test_lanczos_quadrature_host.py runs the same checks from numpy alone)."""
import ctypes as C
import math

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import gram_path_cases as gp
import gram_tangent_cases as tc
import lanczos_value_cases as lv
import pcg_kernel_cases as kc

pytestmark = pytest.mark.gpu

NAN_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def log_elems(max_iterations):
    return kc.PCG_COLS * (1 + 2 * max_iterations)


def split_log(log, max_iterations):
    """(rz0[16], alpha[max_iterations][16], beta[max_iterations][16]) views of one chunk's log"""
    c = kc.PCG_COLS
    return log[:c], log[c:c + max_iterations * c].reshape(max_iterations, c), log[c + max_iterations * c:].reshape(max_iterations, c)


def fitted(ctx, name, rank, **kw):
    cov, x, y = tc.gradient_inputs(name)
    model = ab.gp_from_covariance(cov, context=ctx)
    ds = ab.RegressionDataset(x, y)
    kw.setdefault("tolerance", lv.FIT_TOL)
    return model, ds, model.fit_iterative(ds, preconditioner_rank=rank, **kw)


def download_state(ctx, fit):
    """agp_debug_iterative_state: (n, rank, delta, L (n x rank; rank 0: n x 0))"""
    fn = capi.load_debug().agp_debug_iterative_state
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    dims, delta = np.full(3, -1, dtype=np.int64), np.full(1, np.nan)
    assert fn(ctx._h, fit._h, _p(dims), _p(delta), None, 0, None, 0) == 0
    n, m = int(dims[0]), int(dims[1])
    L = np.full((n + 3, max(m, 1)), np.nan, order="F")
    if m:
        assert dims[2] >= n
        assert fn(ctx._h, fit._h, _p(dims), _p(delta), _p(L), n + 3, None, 0) == 0
        assert np.all(np.isnan(L[n:])) and not np.isnan(L[:n]).any()
    return n, m, float(delta[0]), np.ascontiguousarray(L[:n, :m])


def fit_max_iterations(ctx, fit):
    fn = capi.load_debug().agp_debug_iterative_solve_logged
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_int64, C.c_double, C.c_void_p]
    mi = C.c_int(-1)
    assert fn(ctx._h, fit._h, None, 0, 0, None, 0, None, None, None, 0, 0., C.byref(mi)) == 0
    return fn, mi.value


def solve_logged(ctx, fit, B, tolerance=0.):
    """agp_debug_iterative_solve_logged: (status, X, iterations, residual, [log per chunk], max_iterations); the logs arrive in
    a NaN-filled (all bits set) buffer"""
    fn, mi = fit_max_iterations(ctx, fit)
    n, t = B.shape
    chunks = (t + kc.PCG_COLS - 1) // kc.PCG_COLS
    Bf = np.asfortranarray(B)
    X = np.full((n, t), np.nan, order="F")
    its, res = np.full(t, -7, dtype=np.int32), np.full(t, np.nan)
    log = np.full(chunks * log_elems(mi), np.nan)
    log.view(np.uint64)[:] = NAN_BITS
    out = C.c_int(0)
    st = fn(ctx._h, fit._h, _p(Bf), n, t, _p(X), n, _p(its), _p(res), _p(log), log.size, tolerance, C.byref(out))
    return st, X, its, res, [log[k * log_elems(mi):(k + 1) * log_elems(mi)] for k in range(chunks)], mi


def solve_stepped(ctx, fit, B):
    """agp_debug_iterative_solve_stepped: (status, X, trace (one control block per iteration queued), log, max_iterations)"""
    _, mi = fit_max_iterations(ctx, fit)
    fn = capi.load_debug().agp_debug_iterative_solve_stepped
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                   C.c_void_p, C.c_int64]
    n, t = B.shape
    Bf = np.asfortranarray(B)
    X = np.full((n, t), np.nan, order="F")
    trace = np.zeros(mi, dtype=kc.CTRL)
    log = np.full(log_elems(mi), np.nan)
    log.view(np.uint64)[:] = NAN_BITS
    steps = C.c_int(-1)
    st = fn(ctx._h, fit._h, _p(Bf), n, t, _p(X), n, _p(trace), trace.nbytes, C.byref(steps), _p(log), log.size)
    return st, X, trace[:steps.value], log, mi


def device_probes(ctx, fit, seed, t):
    fn = capi.load_debug().agp_debug_iterative_probes
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p, C.c_int64]
    n = fit.n
    Z = np.full((n + 3, t + 1), np.nan, order="F")
    assert fn(ctx._h, fit._h, seed, t, _p(Z), n + 3) == 0
    assert np.all(np.isnan(Z[n:])) and np.all(np.isnan(Z[:, t])) and not np.isnan(Z[:n, :t]).any()
    return np.ascontiguousarray(Z[:n, :t])


def device_normals(ctx, seed, n, m, t):
    """(G1 m x t, G2 n x t) of the documented probes from agp_standard_normal itself: the bits the probe kernel is fed (the
    device's log and cos round differently from numpy's)"""
    def draw(sd, rows):
        out = np.empty((rows, t), order="F")
        ctx._check(ctx._lib.agp_standard_normal(ctx._h, sd, rows, 0, t, _p(out), rows, capi.HOST), "agp_standard_normal")
        return out
    return (draw(seed ^ lv.FACTOR_SEED, m) if m else np.zeros((0, t))), draw(seed, n)


def c_value(ctx, fm, t, seed=0, probes=None, location=capi.HOST, quadrature_tolerance=0., gradient=False, extra=2):
    """agp_iterative_nll on canary outputs: dict(status, nll, nll_stderr, log_det, samples, grad, grad_stderr, grad_samples,
    iterations, residual, raw = every output buffer whole)"""
    cov = fm.get_model().covariance_function_
    pairs = [(node, param) for node, param, _ in cov.param_slots()[0]] if gradient else []
    P = len(pairs)
    arr = (capi.GradientSlot * max(1, P))(*[capi.GradientSlot(a, b) for a, b in pairs])
    n = fm.get_fit().n
    scal = gp.canaries(3)
    tt = max(t, 1)
    samples = gp.canaries(tt + extra)
    grad, gse = gp.canaries(P + extra), gp.canaries(P + extra)
    lds = tt + extra
    gs = gp.canaries(lds * (P + 1))
    its, res = np.full(tt + extra, -7, dtype=np.int32), gp.canaries(tt + extra)
    zp, ldp, keep = None, 0, None
    if probes is not None and location == capi.DEVICE:
        keep = ctx.to_device(np.ascontiguousarray(np.asarray(probes).T))  # (the bytes of the column-major n x t matrix)
        zp, ldp = C.c_void_p(keep.ptr), n
    elif probes is not None:
        keep = np.asfortranarray(probes)
        zp, ldp = _p(keep), n
    D = C.POINTER(C.c_double)
    sp = [C.cast(C.c_void_p(scal.ctypes.data + 8 * k), D) for k in range(3)]
    st = ctx._lib.agp_iterative_nll(ctx._h, fm.get_fit()._h, t, seed, zp, ldp, location, quadrature_tolerance, P, arr if P else None, None, n,
                                    sp[0], sp[1], sp[2], _p(samples), _p(grad) if P else None, _p(gse) if P else None,
                                    _p(gs) if P else None, lds, _p(its), _p(res))
    S = gs.reshape((lds, P + 1), order="F")
    return dict(status=st, nll=scal[0], nll_stderr=scal[1], log_det=scal[2], samples=samples[:tt].copy(), grad=grad[:P].copy(),
                grad_stderr=gse[:P].copy(), grad_samples=S[:tt, :P].copy(), iterations=its, residual=res,
                raw=(scal, samples, grad, gse, gs))


# ---- 1. the record kernel ---------------------------------------------------------------------------------------------------------------
def record(ctx, ctrl, buf, offset, max_iterations, k, t):
    fn = capi.load_debug().agp_debug_pcg_record
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]
    return fn(ctx._h, _p(ctrl), _p(buf), buf.size, offset, max_iterations, k, t)


def _record_ctrl(active, stopped=()):
    rng = kc.rng_of(77, active)
    ctrl = np.zeros(1, dtype=kc.CTRL)
    ctrl["active"] = active
    ctrl["stopped"][0, list(stopped)] = 1
    for f in ("alpha", "beta", "bb", "resid"):
        ctrl[f][0] = rng.uniform(0.5, 2., kc.PCG_COLS)
    ctrl["rz"][0] = rng.uniform(0.5, 2., (2, kc.PCG_COLS))
    return ctrl


@pytest.mark.parametrize("t", [1, 7, 16])
def test_record_kernel_writes_its_row_and_nothing_else(ctx, t):
    mi, off, tail = 5, 3, 4
    stopped = () if t == 1 else (1, t - 1)
    for k in (0, 3, mi - 1):
        ctrl = _record_ctrl(t - len(stopped), stopped)
        buf = gp.canaries(off + log_elems(mi) + tail)
        want = buf.copy()
        rz0, al, be = split_log(want[off:off + log_elems(mi)], mi)
        for c in range(t):
            if c in stopped:
                continue
            if k == 0:
                rz0[c] = ctrl["rz"][0, 0, c]
            al[k, c], be[k, c] = ctrl["alpha"][0, c], ctrl["beta"][0, c]
        keep = ctrl.copy()
        assert record(ctx, ctrl, buf, off, mi, k, t) == 0
        assert same_bits(buf, want), (t, k)
        assert ctrl.tobytes() == keep.tobytes()
    # no column runs, or an error was marked while three did: nothing is written
    for active in (0, kc.ERROR_ACTIVE):
        buf = gp.canaries(off + log_elems(mi) + tail)
        assert record(ctx, _record_ctrl(active), buf, off, mi, 0, t) == 0
        assert gp.all_canary(buf), active
    # extents are checked before anything is launched
    buf = gp.canaries(off + log_elems(mi) + tail)
    for bad in (dict(k=mi), dict(k=-1), dict(t=0), dict(t=17), dict(offset=tail + off + 1), dict(max_iterations=mi + 1)):
        a = dict(offset=off, max_iterations=mi, k=0, t=t)
        a.update(bad)
        assert record(ctx, _record_ctrl(1), buf, a["offset"], a["max_iterations"], a["k"], a["t"]) == capi.AGP_ERR_INVALID_ARGUMENT, bad
    assert gp.all_canary(buf)


def test_log_rows_are_the_control_block_words_of_a_live_solve(ctx):
    _, _, fm = fitted(ctx, "n65_3d", 16)
    fit = fm.get_fit()
    n = fit.n
    rng = np.random.default_rng(21)
    B = rng.standard_normal((n, 5))
    B[:, 2] = 0.                       # never iterates
    B[:, 3] = np.eye(n)[:, 0]          # a unit vector
    st, X, trace, log, mi = solve_stepped(ctx, fit, B)
    assert st == capi.AGP_OK and len(trace) >= 8
    rz0, al, be = split_log(log, mi)
    iters = trace[-1]["iters"][:5]
    assert iters[2] == 0 and len(set(iters.tolist())) >= 2, iters  # the columns do not all stop together
    for c in range(5):
        for k in range(iters[c]):
            assert _bits(al[k, c]) == _bits(trace[k]["alpha"][c]) and _bits(be[k, c]) == _bits(trace[k]["beta"][c]), (c, k)
        if iters[c]:
            assert _bits(rz0[c]) == _bits(trace[0]["rz"][0, c]) and be[0, c] == 0.
        else:
            assert _bits(rz0[c]) == NAN_BITS
        # a stopped column's later rows, and the columns the chunk does not have, keep their fill
        assert np.all(_bits(al[iters[c]:, c]) == NAN_BITS) and np.all(_bits(be[iters[c]:, c]) == NAN_BITS), c
    assert np.all(_bits(al[:, 5:]) == NAN_BITS) and np.all(_bits(be[:, 5:]) == NAN_BITS) and np.all(_bits(rz0[5:]) == NAN_BITS)
    # the solve with a look after every iteration is the solve: the bits of agp_iterative_solve, whose launches it shares
    assert same_bits(X, fit.solve(B))
    st2, X2, its2, _, logs, _ = solve_logged(ctx, fit, B)
    assert st2 == capi.AGP_OK and same_bits(X2, X) and np.array_equal(its2, iters)
    r2, a2, b2 = split_log(logs[0], mi)
    rows = int(iters.max())
    assert same_bits(a2[:rows], al[:rows]) and same_bits(b2[:rows], be[:rows]) and same_bits(r2, rz0)


def test_a_seventeen_column_solve_logs_its_second_chunk_from_row_zero(ctx):
    _, _, fm = fitted(ctx, "n65_3d", 16)
    fit = fm.get_fit()
    B = np.random.default_rng(22).standard_normal((fit.n, 17))
    st, X, its, res, logs, mi = solve_logged(ctx, fit, B)
    assert st == capi.AGP_OK and len(logs) == 2 and np.all(its > 0) and np.all(res <= lv.FIT_TOL)
    Xs, its_s, _ = fit.solve(B, return_info=True)
    assert same_bits(X, Xs) and np.array_equal(its, its_s)
    st1, X1, its1, _, logs1, _ = solve_logged(ctx, fit, B[:, 16:17])
    assert st1 == capi.AGP_OK and its1[0] == its[16] and same_bits(X1[:, 0], X[:, 16])
    rz0, al, be = split_log(logs[1], mi)
    r1, a1, b1 = split_log(logs1[0], mi)
    k = int(its[16])
    assert same_bits(rz0[:1], r1[:1]) and same_bits(al[:k, 0], a1[:k, 0]) and same_bits(be[:k, 0], b1[:k, 0])
    assert be[0, 0] == 0. and np.all(al[:k, 0] > 0.)
    assert np.all(_bits(al[k:, 0]) == NAN_BITS) and np.all(_bits(al[:, 1:]) == NAN_BITS) and np.all(_bits(rz0[1:]) == NAN_BITS)
    # every column's coefficients are those of the restated recurrence, to the accuracy a recurrence has
    A, _, _ = tc.dense_system("n65_3d")
    n_, m_, delta, L = download_state(ctx, fit)
    P = lv.preconditioner_from(L, delta)
    r0, a0, b0 = split_log(logs[0], mi)
    for c in (0, 15):
        rz, a, b, _ = lv.pcg_coefficients(A, P, B[:, c])
        assert abs(r0[c] - rz) <= 1e-12 * rz and abs(a0[0, c] - a[0]) <= 1e-12 * a[0] and abs(b0[1, c] - b[1]) <= 1e-10 * b[1]


# ---- 2. the probe kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", lv.PROBE_M)
@pytest.mark.parametrize("n", lv.PROBE_N)
def test_probes_against_longdouble(ctx, n, m):
    if not gp.HAVE_LONGDOUBLE:
        pytest.fail("np.longdouble is no wider than float64 here: no reference")
    rng = np.random.default_rng(100 * n + m)
    x = rng.uniform(0., 6., (n, 2))
    y = np.sin(x).sum(axis=1)
    cov = ab.SquaredExponential(1.5, 1.) + ab.IndependentNoise(0.1)
    fit = ab.gp_from_covariance(cov, context=ctx).fit_iterative(ab.RegressionDataset(x, y), preconditioner_rank=m, tolerance=1e-6).get_fit()
    n_, rank, delta, L = download_state(ctx, fit)
    assert n_ == n and rank == min(m, n)
    L = L.reshape(n, rank)
    seed = 0x1234567890ABCDEF + n
    out = {t: device_probes(ctx, fit, seed, t) for t in lv.PROBE_T}
    worst = 0.
    for t, Z in out.items():
        g1, g2 = device_normals(ctx, seed, n, rank, t)
        h1, h2 = lv.normals(seed, n, rank, t)  # the restated generator: the same numbers up to the rounding of log and cos
        assert np.abs(g2 - h2).max() <= 1e-12 and (rank == 0 or np.abs(g1 - h1).max() <= 1e-12)  # (tests/test_prediction_scores_gpu.py)
        want, bound = lv.probe_reference(L, delta, g1, g2)
        err = np.abs(Z.astype(np.longdouble) - want)
        assert np.all(err <= bound), (n, m, t, float((err / bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"n {n} rank {rank}: worst error / gamma(m + 2) bound {worst:.3g}")
    # column c depends on (seed, c) alone: t = 16 is the first 16 columns of t = 17 (a second chunk), t = 1 the first
    assert same_bits(out[16], out[17][:, :16]) and same_bits(out[1], out[17][:, :1])
    assert not same_bits(out[1], device_probes(ctx, fit, seed + 1, 1))


# ---- 3. exact with exhausting probes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rank", lv.EXACT_SHAPES)
def test_exhausting_probes_are_exact(ctx, name, rank):
    tc.identity_case(name)
    model, ds, fm = fitted(ctx, name, rank)
    cov, x, y = tc.gradient_inputs(name)
    n = len(y)
    n_, m, delta, Ld = download_state(ctx, fm.get_fit())
    assert m == rank
    if rank:
        pcd = ab.pivoted_cholesky(cov, ab.Measurement(x), rank, tolerance=1e-12, context=ctx)
        L = np.asarray(pcd.factor)[:, :pcd.rank]
        assert pcd.rank == rank and same_bits(L, Ld.reshape(n, rank))
    else:
        L = np.zeros((n, 0))
    Z = lv.exhausting_probes(L, delta)
    dense_fm = model.fit(ds)
    dense_ld, dense_ll = dense_fm.get_fit().log_determinant, model.log_likelihood(ds)
    _, dense_grad = model.log_likelihood_gradient(ds)
    _, scale = tc.dense_gradient_nll(name)
    ld_np, nll_np = lv.dense_values(name)
    assert abs(dense_ld - ld_np) <= lv.parity_bar(n, ld_np) and abs(-dense_ll - nll_np) <= lv.parity_bar(n, nll_np)
    value, stderr, grad, gstderr = fm.log_likelihood_and_gradient(probes=Z)
    ld, ld_se = fm.get_fit().log_determinant(probes=Z)
    v_only, _ = fm.log_likelihood(probes=Z)
    print(f"{name} rank {rank}: |log det - dense| {abs(ld - dense_ld):.3g}, |value - dense| {abs(value - dense_ll):.3g} "
          f"(bars {lv.parity_bar(n, dense_ld):.3g}, {lv.parity_bar(n, dense_ll):.3g}); iterations "
          f"{fm.value_iterations.min()}..{fm.value_iterations.max()}")
    assert abs(ld - dense_ld) <= lv.parity_bar(n, dense_ld)
    assert abs(value - dense_ll) <= lv.parity_bar(n, dense_ll)
    assert _bits(np.float64(v_only)) == _bits(np.float64(value))  # the value does not depend on the gradient being asked for
    assert set(grad) == set(gstderr) == set(model.get_params())
    for nm in dense_grad:
        a = abs(grad[nm] - dense_grad[nm]) / scale[nm]
        print(f"{name} rank {rank} {nm}: {a:.3g} s_p from the dense gradient")
        assert a <= 1e-8, (nm, grad[nm], dense_grad[nm], scale[nm])
    assert fm.value_iterations.shape == (n + rank,) and np.all(fm.value_iterations > 0) and np.all(fm.value_residual <= lv.FIT_TOL)
    # the caller's probes on the device: the same bits
    h = c_value(ctx, fm, n + rank, probes=Z, gradient=True)
    d = c_value(ctx, fm, n + rank, probes=Z, gradient=True, location=capi.DEVICE)
    assert h["status"] == d["status"] == capi.AGP_OK and all(same_bits(u, v) for u, v in zip(h["raw"], d["raw"]))
    assert _bits(h["nll"]) == _bits(np.float64(-value))


# ---- 4. the seeded estimate ---------------------------------------------------------------------------------------------------------------
def test_seeded_samples_match_their_definition_and_the_estimate_is_usable(ctx):
    name, rank, t, seed = lv.ESTIMATE
    model, ds, fm = fitted(ctx, name, rank)
    fit = fm.get_fit()
    n = fit.n
    n_, m, delta, L = download_state(ctx, fit)
    P = lv.preconditioner_from(L.reshape(n, m), delta)
    Z = device_probes(ctx, fit, seed, t)
    value, stderr, grad, gstderr, samples, gsamples = fm.log_likelihood_and_gradient(num_probes=t, seed=seed, return_samples=True)
    want = lv.value_restated(name, rank, Z, P=P)
    r = np.abs(samples - want["samples"]) / want["scales"]
    print(f"{name} rank {rank} t {t}: worst value sample error {r.max():.3g} of its scale; iterations "
          f"{fm.value_iterations.min()}..{fm.value_iterations.max()} (restated {want['iterations'].min()}..{want['iterations'].max()})")
    assert np.all(r <= lv.SAMPLE_BAR), float(r.max())
    # ... and of u^T log(M) u itself from the dense eigendecomposition, a reference with no recurrence in it
    rx = np.abs(samples - lv.exact_samples(name, P, Z)) / want["scales"]
    print(f"{name}: worst value sample error against the dense eigendecomposition {rx.max():.3g} of its scale")
    assert np.all(rx <= lv.SAMPLE_BAR), float(rx.max())
    gwant, gscale = lv.gradient_samples_restated(name, P, Z)
    assert set(gsamples) == set(gwant)
    for nm in gwant:
        rg = np.abs(gsamples[nm] - gwant[nm]) / gscale[nm]
        assert np.all(rg <= lv.SAMPLE_BAR), (nm, float(rg.max()))
    # the outputs are the stated functions of the samples
    mean = samples.sum() / t
    se = math.sqrt(((samples - mean) ** 2).sum() / (t * (t - 1)))
    ld, ld_se, ld_samples = fit.log_determinant(num_probes=t, seed=seed, return_samples=True)
    assert same_bits(ld_samples, samples)
    assert abs(ld_se - se) <= 1e-12 * se and abs(stderr - 0.5 * se) <= 1e-12 * se
    assert abs(ld - (lv.log_det_p(P) + mean)) <= 1e-10 * (abs(lv.log_det_p(P)) + abs(mean))
    # ... and usable: within four standard errors of the dense values
    dense_ll = model.log_likelihood(ds)
    dense_ld = model.fit(ds).get_fit().log_determinant
    z, zl = abs(value - dense_ll) / stderr, abs(ld - dense_ld) / ld_se
    print(f"{name}: value {value:.6g} +- {stderr:.3g}, dense {dense_ll:.6g}: {z:.2f} standard errors; log det {ld:.6g} +- {ld_se:.3g}, "
          f"dense {dense_ld:.6g}: {zl:.2f}")
    assert z <= 4. and zl <= 4., (z, zl)
    assert ld_se <= 0.01 * abs(dense_ld)  # a loose stderr cannot carry the test above
    _, dense_grad = model.log_likelihood_gradient(ds)
    for nm in dense_grad:
        zg = abs(grad[nm] - dense_grad[nm]) / gstderr[nm]
        print(f"{name} {nm}: {grad[nm]:.6g} +- {gstderr[nm]:.3g}, dense {dense_grad[nm]:.6g}: {zg:.2f} standard errors")
        assert zg <= 4., (nm, zg)
    # a looser quadrature tolerance shortens the recurrences and moves the value by less than its standard error
    loose, _ = fm.log_likelihood(num_probes=t, seed=seed, quadrature_tolerance=1e-4)
    assert fm.value_iterations.max() < want["iterations"].min() and np.all(fm.value_residual <= 1e-4)
    assert abs(loose - value) <= 1e-3 * stderr, (loose, value)


# ---- 5. the interface ---------------------------------------------------------------------------------------------------------------------
def test_interface(ctx):
    model, ds, fm = fitted(ctx, "n65_3d", 16)
    fit = fm.get_fit()
    n = fit.n
    rhs = np.random.default_rng(5).standard_normal((n, 3))
    solve_before = fit.solve(rhs)
    grad_before = fm.log_likelihood_gradient(num_probes=17, seed=9, return_samples=True)
    info = np.empty(n)
    ctx._check(ctx._lib.agp_iterative_fit_download_information(ctx._h, fit._h, _p(info)), "download")
    # one probe: no standard error
    one = c_value(ctx, fm, 1, seed=4, gradient=True)
    assert one["status"] == capi.AGP_OK and math.isnan(one["nll_stderr"]) and np.all(np.isnan(one["grad_stderr"]))
    assert math.isfinite(one["nll"]) and math.isfinite(one["log_det"])
    v1, s1 = fm.log_likelihood(num_probes=1, seed=4)
    assert math.isnan(s1) and _bits(np.float64(v1)) == _bits(np.float64(-one["nll"]))
    # two calls: equal bits, canaries behind every output
    a, b = c_value(ctx, fm, 17, seed=9, gradient=True), c_value(ctx, fm, 17, seed=9, gradient=True)
    assert a["status"] == b["status"] == capi.AGP_OK
    assert all(same_bits(u, v) for u, v in zip(a["raw"], b["raw"])) and np.array_equal(a["iterations"], b["iterations"])
    assert same_bits(a["residual"], b["residual"])
    assert gp.all_canary(a["raw"][1][17:]) and gp.all_canary(a["raw"][2][len(a["grad"]):]) and np.all(a["iterations"][17:] == -7)
    # the probes the entry draws are the ones the probe kernel's entry returns: the caller's copy gives the same bits
    Z = device_probes(ctx, fit, 9, 17)
    for location in (capi.HOST, capi.DEVICE):
        h = c_value(ctx, fm, 17, probes=Z, gradient=True, location=location)
        assert h["status"] == capi.AGP_OK and all(same_bits(u, v) for u, v in zip(a["raw"], h["raw"])), location
    # value only: the samples of the combined call (the solves run at the fit's tolerance in both)
    v = c_value(ctx, fm, 17, seed=9)
    assert v["status"] == capi.AGP_OK and same_bits(v["samples"], a["samples"]) and _bits(v["nll"]) == _bits(a["nll"])
    # malformed arguments: nothing written
    for bad in (dict(t=0), dict(t=-1), dict(quadrature_tolerance=float("nan"))):
        kw = dict(t=4)
        kw.update(bad)
        r = c_value(ctx, fm, kw.pop("t"), **kw)
        assert r["status"] == capi.AGP_ERR_INVALID_ARGUMENT and all(gp.all_canary(x) for x in r["raw"]) and np.all(r["iterations"] == -7)
    with pytest.raises(ValueError):
        fm.log_likelihood(num_probes=0)
    # two iterations are not enough: the status, the iterations, and nothing else
    # (y = 0 converges in 0 iterations whatever max_iterations: the fit exists, its probes cannot be solved)
    _, x, _ = tc.gradient_inputs("n65_3d")
    short = model.fit_iterative(ab.RegressionDataset(x, np.zeros(n)), preconditioner_rank=0, max_iterations=2)
    assert short.get_fit().iterations == 0
    r = c_value(ctx, short, 3, seed=2, gradient=True)
    assert r["status"] == capi.AGP_ERR_NOT_CONVERGED and all(gp.all_canary(x) for x in r["raw"])
    assert np.all(r["iterations"][:3] == 2) and np.all(r["residual"][:3] > 1e-10) and np.all(r["iterations"][3:] == -7)
    for call in (short.log_likelihood, short.log_likelihood_and_gradient, short.get_fit().log_determinant):
        with pytest.raises(ab.NotConvergedError) as e:
            call(num_probes=3, seed=2)
        assert np.all(e.value.iterations == 2) and e.value.status == capi.AGP_ERR_NOT_CONVERGED
    # a NaN probe
    Zn = Z.copy()
    Zn[3, 1] = np.nan
    r = c_value(ctx, fm, 17, probes=Zn, gradient=True)
    assert r["status"] == capi.AGP_ERR_NAN_INPUT and all(gp.all_canary(x) for x in r["raw"])
    with pytest.raises(ab.NanInputError):
        fm.log_likelihood(probes=Zn)
    # the handle is not written: the solve, the gradient entry and the information vector return the bits they returned
    again = np.empty(n)
    ctx._check(ctx._lib.agp_iterative_fit_download_information(ctx._h, fit._h, _p(again)), "download")
    assert same_bits(info, again) and same_bits(info, fit.information)
    assert same_bits(solve_before, fit.solve(rhs))
    grad_after = fm.log_likelihood_gradient(num_probes=17, seed=9, return_samples=True)
    for u, v in zip(grad_before, grad_after):
        assert set(u) == set(v) and all(same_bits(np.asarray(u[k]), np.asarray(v[k])) for k in u)
