"""Shared by tests/test_pcg_bounds_host.py and tests/test_pcg_kernels_gpu.py: the shapes, inputs, references and bounds of the
kernels of csrc/iterative.hip - the conjugate-gradient sweeps and reductions and the Nystrom preconditioner of the
matrix-free fit - each run on its own through agp_debug_pcg, and the whole preconditioner application on live fits through
agp_debug_iterative_state / agp_debug_iterative_precondition (csrc/debug_api.hip).  Nothing here is measured.

Every kernel of iterative.hip and the GPU test that names it (tests/test_pcg_kernels_gpu.py):
    pcg_dot_kernel<DOT_BB>     test_dot_bb
    pcg_dot_kernel<DOT_RZ>     test_dot_rz
    pcg_dot_kernel<DOT_PQ>     test_dot_pq
    pcg_dot_kernel<DOT_RR>     test_dot_rr
    pcg_lt_r_kernel            test_lt_r
    pcg_precond_kernel         test_precond
    pcg_p_kernel               test_p
    pcg_xr_kernel              test_xr
    pcg_diag_stats_kernel      test_diag_stats
    pcg_shift_kernel           test_shift
    pcg_variance_kernel        test_variance
    pcg_apply_preconditioner   test_application_on_live_fits  (lt_r, the two substitutions, precond; delta, L and the factor)
    pcg_solve, the chunk       test_columns_of_a_chunk_are_independent, test_columns_beyond_the_first_chunk

The bounds.  U = 2^-53, gamma(k) = k U / (1 - k U); references in np.longdouble (u = 2^-64, 2^-11 of a rounding).  A sum
of products in which no term passes through more than k roundings - whatever the order - is within gamma(k) sum |a_i b_i|
of the exact one (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); a fused multiply-add drops the
product's rounding and only helps (iterative.hip is compiled with contraction on).  The bound is relative to sum |a| |b|,
not to the result, and every input has signs, so the sums cancel: a dropped element, block or column misses the bound by
orders of magnitude (tests/test_pcg_bounds_host.py shows both directions).  The counts, from the kernels:

  pcg_dot_kernel.  1024 threads; thread i adds the products i, i + 1024, ...: ceil(n / 1024) roundings on its first term
  (the product, then one addition per further term; 0 + p is exact).  Six __shfl_down steps add 64 lanes: 6.  Thread 0
  adds the 16 wave sums from the left: 16 at the most.  gamma(ceil(n / 1024) + 6 + 16) sum |a_i b_i|.
    DOT_BB stores s; DOT_RZ stores s and beta = s / (the other parity's stored value), one correctly rounded division of
    two stored doubles - exact bits.  DOT_PQ stores alpha = rz / s: with s = s_ref (1 + e), |e| <= bound / |s_ref|, and one
    rounding of the division, |alpha - rz / s_ref| <= (bound / |s_ref| + 2 U) |rz / s_ref| to first order.  DOT_RR stores
    sqrt(s) / sqrt(bb): two square roots and a division, each correctly rounded, of an s that the test cannot see - so the
    stored value is within 4 U relative of sqrt(s) / sqrt(bb) for SOME s within the value bound of s_ref, which is
    |resid - sqrt(s_ref / bb)| <= (bound / (2 s_ref) + 4 U) sqrt(s_ref / bb) to first order (the square root halves e).
  pcg_lt_r_kernel.  256 threads, ceil(n / 256) per thread, six shuffle steps, then (w0 + w1) + (w2 + w3): two.  The
    issue's count is ceil(n / 256) + 6 + 3.
  pcg_precond_kernel.  A thread per row adds m products from the left (m roundings on the first), subtracts from R (1),
    divides (1): gamma(m + 4) (|R| + |L| |U|) / delta holds two to spare.  m = 0: (R - 0) / delta is one division, exact bits.
  pcg_p_kernel, pcg_xr_kernel.  z + beta p and x + alpha p: a product and a sum, or one fma - 2 U (|z| + |beta p|) covers
    both to first order; first = 1 copies Z.
  pcg_diag_stats_kernel.  v_i = d_i + yvar_i (1), ceil(n / 1024) per thread, a tree of ten levels over 1024 threads:
    gamma(ceil(n / 1024) + 11) sum |v_i| against the exact sum of d_i + yvar_i.  fmax / fmin of the float64 v_i: exact bits.
  pcg_shift_kernel.  (i == j ? delta : 0) - C: one subtraction of two doubles, exact bits.
  pcg_variance_kernel.  ceil(n / 256) per thread, six shuffle steps, two additions, the subtraction from the prior:
    gamma(ceil(n / 256) + 6 + 4) sum |Kc S| + U |prior|.

The whole application Z = (R - L u) / delta, u = M^-1 L^T R, M = delta I + L^T L, on a live fit.  With t = L^T R computed to
gamma(n) |L|^T |R|, M formed by the GEMM to gamma(n) |L|^T |L|, and the two substitutions against the computed Cholesky
factor of M solving (M + dM) u = t with |dM| <= gamma(3 m + 2) |C| |C^T| (Higham, theorem 10.4), to first order
    e_u = |M^-1| ( gamma(n) |L|^T |R| + gamma(n) (|L|^T |L|) |u| + gamma(3 m + 2) (|C| |C^T|) |u| ),
    E   = [ gamma(m + 4) (|R| + |L| |u|) + |L| e_u ] / delta,
everything in longdouble from the DOWNLOADED L and delta.  At partial rank E / max |Z| is 1e-14 .. 1e-11: a dropped row tile,
column of L or right-hand side misses it by orders of magnitude.  At m = n delta is the 1e-8 floor and R - L u cancels to
about delta |R|: E / max |Z| is about 1e-5 there.  Those cases stay for their edges (m = n = 2, m = 65 = one block of 64 and
one column, the floor of delta) - they show that nothing is dropped or misaddressed, and are NO evidence of accuracy.

Buffers.  Every matrix sits in a NaN-filled buffer whose leading dimension exceeds its rows, followed by one more NaN
column and three NaN words: an over-read shows as a NaN result or as ctrl.nan, an over-write as a changed sentinel.  Every
case is also run with active = 0 and with active = 3 - PCG_ERROR (an error was marked while three columns ran): every
output keeps every bit, except under DOT_BB, which always runs.  Where a kernel reads stopped[], columns are marked
stopped and keep their bits.
"""
import numpy as np

import iterative_fit_cases as ic
from gram_path_cases import HAVE_LONGDOUBLE  # noqa: F401  (the host test asserts it)

U = 2.0 ** -53
LD = np.longdouble

# csrc/iterative_internal.h
PCG_COLS, PCG_LOOK, PCG_DOT_THREADS, PCG_ERROR = 16, 8, 1024, 1 << 20
DOT_BB, DOT_RZ, DOT_PQ, DOT_RR = range(4)
DOT_NAMES = ["bb", "rz", "pq", "rr"]
CTRL = np.dtype([("active", "<i4"), ("npd", "<i4"), ("nan", "<i4"), ("pad", "<i4"), ("stopped", "<i4", (PCG_COLS,)),
                 ("iters", "<i4", (PCG_COLS,)), ("bb", "<f8", (PCG_COLS,)), ("rz", "<f8", (2, PCG_COLS)), ("alpha", "<f8", (PCG_COLS,)),
                 ("beta", "<f8", (PCG_COLS,)), ("resid", "<f8", (PCG_COLS,))], align=True)
CTRL_FIELDS = ["active", "npd", "nan", "pad", "stopped", "iters", "bb", "rz", "alpha", "beta", "resid"]
# ops of agp_debug_pcg (csrc/debug_api.hip); the four dot modes are ops 0 .. 3
OP_DOT, OP_LT_R, OP_PRECOND, OP_P, OP_XR, OP_DIAG_STATS, OP_SHIFT, OP_VARIANCE = 0, 4, 5, 6, 7, 8, 9, 10
ERROR_ACTIVE = 3 - PCG_ERROR


def ctrl_layout():
    """what agp_debug_pcg_ctrl_layout returns for the mirror above"""
    return [CTRL.itemsize] + [CTRL.fields[f][1] for f in CTRL_FIELDS] + [PCG_COLS, PCG_LOOK, PCG_DOT_THREADS, PCG_ERROR]


def gamma(k):
    return k * U / (1. - k * U)


def rng_of(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ---- shapes -----------------------------------------------------------------------------------------------------------
DOT_N = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 3000]
DOT_T = [1, 16]
LT_R_N = [1, 63, 64, 255, 256, 257, 513, 1025]
LT_R_M = [1, 2, 65]
LT_R_T = [1, 5, 16]
PRECOND_N = [1, 255, 256, 257, 513]
PRECOND_M = [0, 1, 65]
PRECOND_T = [1, 5, 16]
SWEEP_N = [1, 255, 256, 257, 513]
SWEEP_T = [1, 16]
STATS_N = [1, 1023, 1024, 1025, 3000]
SHIFT_M = [1, 2, 255, 256, 257]
VARIANCE_N = [1, 255, 256, 257, 1025]
VARIANCE_T = [1, 16]
RR_TOL = 1e-6  # the tolerance of the DOT_RR stop cases


def stopped_sets(t):
    """the stop marks a case is run with where its kernel reads stopped[]"""
    return [(), (0,)] if t == 1 else [(1, t - 1)]


def dot_counts(n):
    return -(-n // PCG_DOT_THREADS) + 6 + 16


def lt_r_counts(n):
    return -(-n // 256) + 6 + 3


def variance_counts(n):
    return -(-n // 256) + 6 + 4


def stats_counts(n):
    return -(-n // 1024) + 11


# ---- buffers ------------------------------------------------------------------------------------------------------------
def padded(M, ld):
    """Column-major rows x cols M in a NaN-filled buffer of leading dimension ld > rows with one more column and three more
    words, all NaN: (flat, the rows x cols view)."""
    M = np.asarray(M, dtype=np.float64)
    rows, cols = M.shape
    assert ld > rows
    flat = np.full(ld * (cols + 1) + 3, np.nan)
    view = flat[:ld * cols].reshape((ld, cols), order="F")[:rows]
    view[:] = M
    return flat, view


def vector(v, extra=3):
    flat = np.full(len(v) + extra, np.nan)
    flat[:len(v)] = v
    return flat, flat[:len(v)]


def fresh_ctrl(rng, t, active, stopped=()):
    """A control block (a one-element CTRL array and the byte buffer that holds it, 16 sentinel bytes behind) whose every
    field has a value of its own: what a kernel must not write is compared bit for bit afterwards."""
    raw = np.full(CTRL.itemsize + 16, 0xA5, dtype=np.uint8)
    c = raw[:CTRL.itemsize].view(CTRL)
    c["active"], c["npd"], c["nan"], c["pad"] = active, 0, 0, 0
    c["stopped"] = 0
    for s in stopped:
        c["stopped"][0, s] = 1
    c["iters"] = 100 + np.arange(PCG_COLS)
    for f in ("bb", "rz", "alpha", "beta", "resid"):
        c[f] = rng.standard_normal(c[f].shape)
    c["bb"] = np.abs(c["bb"]) + 0.5
    return c, raw


# ---- sums of products: canonical form, reference, bound, plain evaluations --------------------------------------------------
def sum_reference(F0, F1):
    """(sum_k F0[o, k] F1[o, k] in longdouble, sum_k |F0 F1|) for every output o"""
    P = F0.astype(LD) * F1.astype(LD)
    return P.sum(axis=1), np.abs(F0 * F1).sum(axis=1)


def error_ratio(got, ref, bound):
    """max |got - ref| / bound; a zero bound admits only an exact result; a NaN or an infinity is infinitely wrong"""
    got, bound = np.asarray(got).reshape(-1), np.asarray(bound, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref).reshape(-1)
    err = np.abs(got.astype(LD) - ref.astype(LD)).astype(np.float64)
    if not np.all(np.isfinite(err)):
        return np.inf
    zero = bound == 0.
    if np.any(err[zero] != 0.):
        return np.inf
    return float((err[~zero] / bound[~zero]).max()) if np.any(~zero) else 0.


def plain_sum(F0, F1):
    """numpy's own summation (the wrong results below are built with it: they miss the bounds by orders, not by an order)"""
    return np.einsum("ok,ok->o", F0, F1)


def kernel_sum(F0, F1, threads, final):
    """Plain fp64 in the kernels' order: thread i adds the products i, i + threads, ... from the left (a rounded product and a
    rounded sum: one more rounding per step than the kernels' fma, within the same count per term); then `final`:
    "waves_left" - six halving steps inside every 64 lanes, the wave sums from the left (pcg_dot_kernel);
    "waves_pairs" - the same, then (w0 + w1) + (w2 + w3) (pcg_lt_r_kernel, pcg_variance_kernel; threads = 256);
    "tree" - halving steps over all the threads (pcg_diag_stats_kernel)."""
    o, n = F0.shape
    passes = -(-n // threads)
    P = np.zeros((o, passes * threads))
    P[:, :n] = F0 * F1  # (adding a zero is exact: the threads past n hold 0)
    P = P.reshape(o, passes, threads)
    acc = np.zeros((o, threads))
    for k in range(passes):
        acc = acc + P[:, k]
    if final == "tree":
        w = threads // 2
        while w > 0:
            acc = acc[:, :w] + acc[:, w:2 * w]
            w //= 2
        return acc[:, 0]
    acc = acc.reshape(o, threads // 64, 64)
    off = 32
    while off > 0:
        acc = acc[:, :, :off] + acc[:, :, off:2 * off]
        off //= 2
    waves = acc[:, :, 0]
    if final == "waves_pairs":
        return (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])
    s = np.zeros(o)
    for w in range(waves.shape[1]):
        s = s + waves[:, w]
    return s


def wrong_sums(F0, F1, block):
    """the results the GPU tests are there to refuse: {what: plain fp64 sums}"""
    n = F0.shape[1]
    cut = (n - 1) // block * block  # the first term of the last block of `block` terms
    out = {"last element dropped": plain_sum(F0[:, :-1], F1[:, :-1]),
           "a term counted twice": plain_sum(F0, F1) + F0[:, -1] * F1[:, -1],
           "column shifted by one": plain_sum(np.roll(F0, 1, axis=1), F1)}
    if cut > 0:
        out[f"last block of {block} dropped"] = plain_sum(F0[:, :cut], F1[:, :cut])
    return out


# ---- pcg_dot_kernel -----------------------------------------------------------------------------------------------------------
def dot_cases():
    return [dict(id=f"n{n}-t{t}", n=n, t=t) for n in DOT_N for t in DOT_T]


def dot_problem(mode, case):
    """a, b (n x t, standard normal; DOT_BB and DOT_RR: b is a) and, for DOT_PQ, the sign of b's columns chosen so that the
    exact sum is positive (the terms still cancel)."""
    n, t = case["n"], case["t"]
    rng = rng_of(n, t, mode, 11)
    a = rng.standard_normal((n, t))
    b = a if mode in (DOT_BB, DOT_RR) else rng.standard_normal((n, t))
    if mode == DOT_PQ:
        s, _ = sum_reference(a.T, b.T)
        b = b * np.where(s < 0, -1., 1.)
    ref, mag = sum_reference(a.T, b.T)
    return dict(a=a, b=b, ref=ref, bound=gamma(dot_counts(n)) * mag)


# ---- pcg_lt_r_kernel ----------------------------------------------------------------------------------------------------------
def lt_r_cases():
    return [dict(id=f"n{n}-m{m}-t{t}", n=n, m=m, t=t) for n in LT_R_N for m in LT_R_M for t in LT_R_T]


def lt_r_problem(case):
    n, m, t = case["n"], case["m"], case["t"]
    rng = rng_of(n, m, t, 12)
    L, R = rng.standard_normal((n, m)), rng.standard_normal((n, t))
    ref = L.T.astype(LD) @ R.astype(LD)
    return dict(L=L, R=R, ref=ref, bound=gamma(lt_r_counts(n)) * (np.abs(L).T @ np.abs(R)))


def lt_r_canonical(p):
    """(F0, F1): output j + m c, terms i"""
    m, t = p["L"].shape[1], p["R"].shape[1]
    return np.tile(p["L"].T, (t, 1)), np.repeat(p["R"].T, m, axis=0)


# ---- pcg_precond_kernel -------------------------------------------------------------------------------------------------------
def precond_cases():
    return [dict(id=f"n{n}-m{m}-t{t}", n=n, m=m, t=t) for n in PRECOND_N for m in PRECOND_M for t in PRECOND_T]


def precond_problem(case):
    n, m, t = case["n"], case["m"], case["t"]
    rng = rng_of(n, m, t, 13)
    L, Um, R = rng.standard_normal((n, m)), rng.standard_normal((m, t)), rng.standard_normal((n, t))
    delta = 0.37
    ref = (R.astype(LD) - L.astype(LD) @ Um.astype(LD)) / LD(delta)
    bound = gamma(m + 4) * (np.abs(R) + np.abs(L) @ np.abs(Um)) / delta
    return dict(L=L, U=Um, R=R, delta=delta, ref=ref, bound=bound)


# ---- pcg_p_kernel, pcg_xr_kernel ----------------------------------------------------------------------------------------------
def sweep_cases():
    return [dict(id=f"n{n}-t{t}", n=n, t=t) for n in SWEEP_N for t in SWEEP_T]


def sweep_problem(case):
    """X, R, P, Q, Z (n x t) and the alpha and beta of the t columns"""
    n, t = case["n"], case["t"]
    rng = rng_of(n, t, 14)
    p = {k: rng.standard_normal((n, t)) for k in ("X", "R", "P", "Q", "Z")}
    p["alpha"], p["beta"] = rng.standard_normal(t), rng.standard_normal(t)
    return p


def axpy_reference(x, a, p):
    """(x + a p in longdouble, 2 U (|x| + |a p|)), a per column"""
    ap = a.astype(LD)[None, :] * p.astype(LD)
    return x.astype(LD) + ap, 2. * U * (np.abs(x) + np.abs(ap).astype(np.float64))


# ---- pcg_diag_stats_kernel ----------------------------------------------------------------------------------------------------
def stats_cases():
    """n, with and without yvar, and where the maximum and the minimum sit: index 0, n - 1 and 1024 (the first element of a
    thread's second pass) in turn"""
    out = []
    for n in STATS_N:
        places = sorted({0, n - 1} | ({1024} if n > 1024 else set()))
        for yvar in (False, True):
            for k, pmax in enumerate(places):
                pmin = places[(k + 1) % len(places)]
                out.append(dict(id=f"n{n}-yvar{int(yvar)}-max{pmax}-min{pmin}", n=n, yvar=yvar, pmax=pmax, pmin=pmin))
    return out


def stats_problem(case):
    n = case["n"]
    rng = rng_of(n, case["pmax"], case["pmin"], int(case["yvar"]), 15)
    d = rng.uniform(0.5, 2., n)
    yvar = rng.uniform(0.02, 0.2, n) if case["yvar"] else None
    d[case["pmin"]] = 0.01 + rng.uniform(0., 0.001)
    d[case["pmax"]] = 10. + rng.uniform(0., 1.)  # (n = 1: one element is both)
    v = d + (yvar if yvar is not None else 0.)
    exact = d.astype(LD) + (yvar.astype(LD) if yvar is not None else LD(0.))
    return dict(d=d, yvar=yvar, v=v, max=v.max(), min=v.min(), ref=exact.sum(), bound=gamma(stats_counts(n)) * np.abs(v).sum())


# ---- pcg_shift_kernel ---------------------------------------------------------------------------------------------------------
def shift_problem(m):
    rng = rng_of(m, 16)
    Cm = rng.standard_normal((m, m))
    Cm[0, 0] = 0.  # (delta - 0 and 0 - 0)
    if m > 1:
        Cm[1, 0] = 0.
    delta = 0.0123
    return dict(C=Cm, delta=delta, want=np.where(np.eye(m, dtype=bool), delta, 0.) - Cm)


# ---- pcg_variance_kernel ------------------------------------------------------------------------------------------------------
def variance_cases():
    return [dict(id=f"n{n}-t{t}", n=n, t=t) for n in VARIANCE_N for t in VARIANCE_T]


def variance_problem(case):
    n, t = case["n"], case["t"]
    rng = rng_of(n, t, 17)
    Kc, S = rng.standard_normal((n, t)), rng.standard_normal((n, t))
    prior = rng.uniform(0.5, 2., t)
    s, mag = sum_reference(Kc.T, S.T)
    return dict(Kc=Kc, S=S, prior=prior, ref=prior.astype(LD) - s, bound=gamma(variance_counts(n)) * mag + U * np.abs(prior))


# ---- the whole application on live fits ---------------------------------------------------------------------------------------
# (fit of iterative_fit_cases, preconditioner ranks)
LIVE_FITS = [("n777_2d", (1, 16, 64)), ("n65_3d", (64, 65)), ("n2", (2,))]
LIVE_T = [1, 16]
LIVE_STOPPED = {1: (), 16: (2, 15)}
PRECOND_REL_TOL = 1e-12  # the default of fit_iterative


def live_cases():
    return [dict(id=f"{name}-rank{r}-{'var' if v else 'no_var'}", name=name, rank=r, with_var=v)
            for name, ranks in LIVE_FITS for r in ranks for v in (False, True)]


def live_rhs(n, t, rank):
    return np.asfortranarray(rng_of(n, t, rank, 18).standard_normal((n, t)))


def delta_reference(diag, L):
    """(delta from the definition with the trace in longdouble, its bound gamma(n + m n) sum A_ii)"""
    n, m = L.shape
    floor = ic.DELTA_FLOOR * diag.max()
    trace = diag.astype(LD).sum() - (L.astype(LD) ** 2).sum()
    ref = max(float(trace / LD(n - m)), floor) if m < n else floor
    return ref, gamma(n + m * n) * float(diag.sum())


def _cholesky_ld(M):
    m = M.shape[0]
    Cm = np.zeros((m, m), dtype=LD)
    for j in range(m):
        d = M[j, j] - (Cm[j, :j] ** 2).sum()
        assert d > 0
        Cm[j, j] = np.sqrt(d)
        if j + 1 < m:
            Cm[j + 1:, j] = (M[j + 1:, j] - Cm[j + 1:, :j] @ Cm[j, :j]) / Cm[j, j]
    return Cm


def _lower_inverse_ld(Cm):
    m = Cm.shape[0]
    X = np.zeros((m, m), dtype=LD)
    for i in range(m):
        e = np.zeros(m, dtype=LD)
        e[i] = 1
        X[i] = (e - Cm[i, :i] @ X[:i]) / Cm[i, i]
    return X


class Application:
    """Z = P^-1 R of the preconditioner (L, delta) in longdouble, with the componentwise bound E of the module docstring"""

    def __init__(self, L, delta):
        self.L, self.delta = np.asarray(L, dtype=np.float64), float(delta)
        self.n, self.m = self.L.shape
        if self.m:
            Ll = self.L.astype(LD)
            self.M = LD(self.delta) * np.eye(self.m, dtype=LD) + Ll.T @ Ll
            self.C = _cholesky_ld(self.M)
            Ci = _lower_inverse_ld(self.C)
            self.Minv = Ci.T @ Ci
            self.absLtL = np.abs(Ll).T @ np.abs(Ll)
            self.absCCt = np.abs(self.C) @ np.abs(self.C).T

    def reference(self, R):
        """(Z, E) for R (n x t)"""
        Rl = np.asarray(R, dtype=np.float64).astype(LD)
        if not self.m:
            Z = Rl / LD(self.delta)
            return Z, (gamma(4) * np.abs(Z)).astype(np.float64)
        Ll, aL, aR = self.L.astype(LD), np.abs(self.L).astype(LD), np.abs(Rl)
        u = self.Minv @ (Ll.T @ Rl)
        Z = (Rl - Ll @ u) / LD(self.delta)
        au = np.abs(u)
        n, m = self.n, self.m
        e_u = np.abs(self.Minv) @ (gamma(n) * (aL.T @ aR) + gamma(n) * (self.absLtL @ au) + gamma(3 * m + 2) * (self.absCCt @ au))
        E = (gamma(m + 4) * (aR + aL @ au) + aL @ e_u) / LD(self.delta)
        return Z, E.astype(np.float64)

    def factor_bound(self):
        """(M, bound): the computed Cholesky factor C of the computed M has |C C^T - M| <= gamma(n) |L|^T |L| +
        gamma(m + 1) |C| |C^T| (the GEMM that formed M and the shift: n + 1 roundings a term at the most, taken into
        gamma(n) |L|^T |L| + U delta; Higham, theorem 10.3), to first order with the exact factor's |C| |C^T|"""
        return self.M, (gamma(self.n) * self.absLtL + gamma(self.m + 1) * self.absCCt + U * self.delta * np.eye(self.m)).astype(np.float64)


def plain_application(L, delta, R):
    """the same in plain float64: numpy's products, LAPACK's Cholesky and solves"""
    if not L.shape[1]:
        return R / delta
    chol = np.linalg.cholesky(delta * np.eye(L.shape[1]) + L.T @ L)
    u = np.linalg.solve(chol.T, np.linalg.solve(chol, L.T @ R))
    return (R - L @ u) / delta


# ---- the columns of a chunk -----------------------------------------------------------------------------------------------------
INDEPENDENCE_FIT = "n777_2d"
INDEPENDENCE_RANKS = [0, 64]
POSITIONS = [0, 7, 15]
DEVICE_GAP, HOST_GAP = 2 * PCG_LOOK, 20


def independence_vectors(A, rank):
    """The column under test and its neighbours for the fit of INDEPENDENCE_FIT with y_var at preconditioner rank `rank`:
    dict(test, early = [columns that stop at least two looks of the host before it], late = [columns that run at least two
    looks longer]).  rank 0: the sum of the top 24 eigenvectors of A (24 distinct eigenvalues: about 24 iterations of plain
    CG), a single eigenvector (1 iteration) and zero (0) before it, standard-normal vectors (hundreds) behind it.  rank 64:
    the top eigenvector (the preconditioner has flattened the top of the spectrum, not one eigenvector: tens of iterations),
    zero before it, standard-normal vectors behind."""
    n = A.shape[0]
    V = np.linalg.eigh(A)[1][:, ::-1]  # the top eigenvector first
    rng = rng_of(n, rank, 19)
    normals = [rng.standard_normal(n) for _ in range(4)]
    zero = np.zeros(n)
    if rank == 0:
        return dict(test=V[:, :24].sum(axis=1), early=[V[:, 30].copy(), zero, V[:, 3].copy()], late=normals)
    return dict(test=V[:, 0].copy(), early=[zero], late=normals)


def chunk_around(vs, c, variant):
    """16 columns with the column under test at position c; the other positions filled in turn with the early and the late
    neighbours, `variant` choosing where the turn starts and which neighbours come first."""
    n = len(vs["test"])
    B = np.zeros((n, PCG_COLS), order="F")
    fill = []
    early, late = vs["early"], vs["late"]
    for k in range(PCG_COLS):
        pool = early if (k + variant) % 2 == 0 else late
        fill.append(pool[(k // 2 + variant) % len(pool)])
    for k in range(PCG_COLS):
        B[:, k] = vs["test"] if k == c else fill[k]
    return B
