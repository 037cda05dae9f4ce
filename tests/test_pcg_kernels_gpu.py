"""Every kernel of csrc/iterative.hip on its own through agp_debug_pcg - the launchers of csrc/iterative_internal.h, i.e. the
grid and block arithmetic the product runs - the whole preconditioner application on live fits through
agp_debug_iterative_state / agp_debug_iterative_precondition, and the independence of the right-hand sides of a chunk
through the public solve (csrc/debug_api.hip; include/albatross_amd.h).

Shapes, inputs, references and bounds are tests/pcg_kernel_cases.py's (its docstring derives the bounds and lists which test
names which kernel; tests/test_pcg_bounds_host.py shows that plain fp64 evaluations meet them on these inputs and that a
dropped, doubled or shifted term does not).  Sums assert error / bound <= 1 against a longdouble reference; what a kernel
must not write - the control block's other fields, stopped columns, padding rows, the column and the words behind a
buffer, every output of a launch that finds active <= 0 - is compared bit for bit.  Each test prints its worst ratio."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import iterative_fit_cases as ic
import pcg_kernel_cases as kc

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 1  # include/albatross_amd.h: AGP_ERR_INVALID_ARGUMENT
NAN_BITS = np.array([np.nan]).view(np.uint64)[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want))


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def pcg_call(ctx, op, ip, dp, bufs):
    """agp_debug_pcg: bufs are flat numpy arrays (run in place) or None; the same array twice shares a device buffer."""
    fn = capi.load_debug().agp_debug_pcg
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    for b in bufs:
        assert b is None or (b.flags.c_contiguous and b.flags.writeable and b.ndim == 1)
    ipa = np.asarray(ip, dtype=np.int64)
    dpa = np.asarray(dp, dtype=np.float64)
    ptrs = (C.c_void_p * len(bufs))(*[None if b is None else b.ctypes.data for b in bufs])
    sizes = np.asarray([0 if b is None else b.nbytes for b in bufs], dtype=np.int64)
    return fn(ctx._h, op, ipa.ctypes.data, len(ipa), dpa.ctypes.data if len(dpa) else None, len(dpa), ptrs, sizes.ctypes.data, len(bufs))


def run(ctx, op, ip, dp, bufs, read_only=()):
    """one launch; the buffers at the positions `read_only` come back with the bits they had"""
    keep = {k: bufs[k].copy() for k in read_only if bufs[k] is not None}
    st = pcg_call(ctx, op, ip, dp, bufs)
    assert st == 0, st
    for k, was in keep.items():
        assert same_bits(bufs[k], was), f"buffer {k} was written"


def inert(ctx, op, ip, dp, make):
    """make(active) -> the buffers of a launch, the control block first.  With active = 0 and with an error marked while
    three columns ran, every buffer keeps every bit."""
    for active in (0, kc.ERROR_ACTIVE):
        bufs = make(active)
        run(ctx, op, ip, dp, bufs, read_only=range(len(bufs)))


def view(flat, ld, rows, cols):
    return flat[:ld * cols].reshape((ld, cols), order="F")[:rows]


def only_written(flat, before, ld, rows, cols, skip_cols=()):
    """outside the rows x cols block (and in its columns `skip_cols`) flat has the bits of `before`"""
    a, b = flat.copy(), before.copy()
    for c in range(cols):
        if c not in skip_cols:
            view(a, ld, rows, cols)[:, c] = 0.
            view(b, ld, rows, cols)[:, c] = 0.
    return same_bits(a, b)


def test_control_block_layout():
    """the mirror of PcgCtrl every other test reads the control block through"""
    out = np.full(16, -1, dtype=np.int64)
    fn = capi.load_debug().agp_debug_pcg_ctrl_layout
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert fn(_p(out), 16) == 0 and list(out) == kc.ctrl_layout(), (list(out), kc.ctrl_layout())
    assert fn(_p(out), 15) == INVALID_ARGUMENT


# ---- pcg_dot_kernel -----------------------------------------------------------------------------------------------------------
def dot_buffers(mode, p, n):
    a = kc.padded(p["a"], n + 3)[0]
    b = a if mode in (kc.DOT_BB, kc.DOT_RR) else kc.padded(p["b"], n + 3)[0]
    return a, b


def expect_ctrl(c, want, raw):
    """the control block is `want` bit for bit, and the bytes behind it are untouched"""
    for f in kc.CTRL_FIELDS:
        assert same_bits(c[f], want[f]), (f, c[f], want[f])
    assert np.all(raw[kc.CTRL.itemsize:] == 0xA5)


def test_dot_bb(ctx):
    worst = 0.0
    for case in kc.dot_cases():
        n, t = case["n"], case["t"]
        for zero in ([(), (0,)] if t == 1 else [(5,)]):
            for active0 in (0, kc.ERROR_ACTIVE):  # DOT_BB always runs
                p = kc.dot_problem(kc.DOT_BB, case)
                p["a"] = p["a"].copy()
                p["a"][:, list(zero)] = 0.
                a, b = dot_buffers(kc.DOT_BB, p, n)
                c, raw = kc.fresh_ctrl(kc.rng_of(n, t, 1), t, active0)
                want = c.copy()
                run(ctx, kc.OP_DOT + kc.DOT_BB, [n + 3, n, t, 0], [1e-10], [raw, a, b], read_only=(1,))
                ref, mag = kc.sum_reference(p["a"].T, p["a"].T)
                ratio = kc.error_ratio(c["bb"][0, :t], ref, kc.gamma(kc.dot_counts(n)) * mag)
                assert ratio <= 1.0, (case["id"], ratio)
                worst = max(worst, ratio)
                want["bb"][0, :t] = c["bb"][0, :t]
                want["resid"][0, :t] = [0. if k in zero else 1. for k in range(t)]
                want["stopped"][0, list(zero)] = 1
                want["active"] = active0 + t - len(zero)
                expect_ctrl(c, want, raw)
    print(f"dot bb: worst error / bound {worst:.3g}")


def test_dot_rz(ctx):
    worst = 0.0
    for case in kc.dot_cases():
        n, t = case["n"], case["t"]
        p = kc.dot_problem(kc.DOT_RZ, case)
        for stopped in kc.stopped_sets(t):
            live = [k for k in range(t) if k not in stopped]
            for k in (0, 3, 4):
                a, b = dot_buffers(kc.DOT_RZ, p, n)
                c, raw = kc.fresh_ctrl(kc.rng_of(n, t, k, 2), t, t, stopped)
                want = c.copy()
                run(ctx, kc.OP_DOT + kc.DOT_RZ, [n + 3, n, t, k], [1e-10], [raw, a, b], read_only=(1, 2))
                got = c["rz"][0, k & 1, live]
                ratio = kc.error_ratio(got, p["ref"][live], p["bound"][live]) if live else 0.0
                assert ratio <= 1.0, (case["id"], k, ratio)
                worst = max(worst, ratio)
                want["rz"][0, k & 1, live] = got
                want["beta"][0, live] = 0. if k == 0 else got / want["rz"][0, (k - 1) & 1, live]
                expect_ctrl(c, want, raw)
        inert(ctx, kc.OP_DOT + kc.DOT_RZ, [n + 3, n, t, 3], [1e-10],
              lambda active: [kc.fresh_ctrl(kc.rng_of(n, t, 3), t, active)[1], *dot_buffers(kc.DOT_RZ, p, n)])
    print(f"dot rz: worst error / bound {worst:.3g}")


def test_dot_pq(ctx):
    worst = worst_alpha = 0.0
    for case in kc.dot_cases():
        n, t = case["n"], case["t"]
        p = kc.dot_problem(kc.DOT_PQ, case)
        for stopped in kc.stopped_sets(t):
            live = [k for k in range(t) if k not in stopped]
            for k in (0, 3):
                a, b = dot_buffers(kc.DOT_PQ, p, n)
                c, raw = kc.fresh_ctrl(kc.rng_of(n, t, k, 3), t, t, stopped)
                want = c.copy()
                run(ctx, kc.OP_DOT + kc.DOT_PQ, [n + 3, n, t, k], [1e-10], [raw, a, b], read_only=(1, 2))
                if live:
                    rz = want["rz"][0, k & 1, live]
                    ref = rz.astype(kc.LD) / p["ref"][live]
                    tol = (p["bound"][live] / np.abs(p["ref"][live]).astype(np.float64) + 2 * kc.U) * np.abs(ref).astype(np.float64)
                    ratio = kc.error_ratio(c["alpha"][0, live], ref, tol)
                    assert ratio <= 1.0, (case["id"], k, ratio)
                    worst_alpha = max(worst_alpha, ratio)
                    # the sum itself, as far as alpha shows it: s = rz / alpha to two more roundings
                    s = rz.astype(kc.LD) / c["alpha"][0, live].astype(kc.LD)
                    worst = max(worst, kc.error_ratio(s.astype(np.float64), p["ref"][live],
                                                      p["bound"][live] + 2 * kc.U * np.abs(p["ref"][live]).astype(np.float64)))
                    want["alpha"][0, live] = c["alpha"][0, live]
                expect_ctrl(c, want, raw)
        # p^T A p <= 0 in the last column: an exactly zero p, and a q of the wrong sign
        for what in ("zero", "flipped"):
            q = dict(a=p["a"].copy(), b=p["b"].copy())
            if what == "zero":
                q["a"][:, t - 1] = 0.
            else:
                q["b"][:, t - 1] = -q["b"][:, t - 1]
            a, b = dot_buffers(kc.DOT_PQ, q, n)
            c, raw = kc.fresh_ctrl(kc.rng_of(n, t, 33), t, t)
            was = c.copy()
            run(ctx, kc.OP_DOT + kc.DOT_PQ, [n + 3, n, t, 2], [1e-10], [raw, a, b], read_only=(1, 2))
            assert c["npd"][0] == 1 and c["nan"][0] == 0 and c["active"][0] == t - kc.PCG_ERROR, (case["id"], what)
            assert same_bits(c["alpha"][0, t - 1:], was["alpha"][0, t - 1:])
        inert(ctx, kc.OP_DOT + kc.DOT_PQ, [n + 3, n, t, 3], [1e-10],
              lambda active: [kc.fresh_ctrl(kc.rng_of(n, t, 3), t, active)[1], *dot_buffers(kc.DOT_PQ, p, n)])
    assert worst <= 1.0, worst
    print(f"dot pq: alpha, worst error / tolerance {worst_alpha:.3g}; the sum behind it, worst error / bound {worst:.3g}")


def test_dot_rr(ctx):
    worst = 0.0
    tol = kc.RR_TOL
    for case in kc.dot_cases():
        n, t = case["n"], case["t"]
        p = kc.dot_problem(kc.DOT_RR, case)
        for stopped in kc.stopped_sets(t):
            live = [k for k in range(t) if k not in stopped]
            a, b = dot_buffers(kc.DOT_RR, p, n)
            c, raw = kc.fresh_ctrl(kc.rng_of(n, t, 4), t, t, stopped)
            want = c.copy()
            k = 6
            run(ctx, kc.OP_DOT + kc.DOT_RR, [n + 3, n, t, k], [tol], [raw, a, b])
            assert same_bits(a, kc.padded(p["a"], n + 3)[0])
            if live:
                bb = want["bb"][0, live]
                ref = np.sqrt(p["ref"][live] / bb.astype(kc.LD))
                rel = p["bound"][live] / (2 * p["ref"][live].astype(np.float64)) + 4 * kc.U
                ratio = kc.error_ratio(c["resid"][0, live], ref, rel * ref.astype(np.float64))
                assert ratio <= 1.0, (case["id"], ratio)
                worst = max(worst, ratio)
                edge = ref.astype(np.float64) / tol
                assert np.all((edge < 0.99) | (edge > 1.01)), "an input at the rounding edge of the stop rule"
                stops = [col for col, e in zip(live, edge) if e < 1.]
                want["resid"][0, live] = c["resid"][0, live]
                want["iters"][0, live] = k + 1
                want["stopped"][0, stops] = 1
                want["active"] = t - len(stops)
            expect_ctrl(c, want, raw)
        # the stop rule: ||r|| a factor 2 below tol ||b|| (even columns) and a factor 2 above it (odd columns)
        c, raw = kc.fresh_ctrl(kc.rng_of(n, t, 5), t, t)
        want = c.copy()
        norm = np.sqrt(p["ref"]).astype(np.float64)
        factor = np.where(np.arange(t) % 2 == 0, 0.5, 2.)
        scaled = p["a"] * (factor * tol * np.sqrt(want["bb"][0, :t]) / norm)[None, :]
        a = kc.padded(scaled, n + 3)[0]
        run(ctx, kc.OP_DOT + kc.DOT_RR, [n + 3, n, t, 0], [tol], [raw, a, a])
        want["stopped"][0, :t] = np.arange(t) % 2 == 0
        want["active"] = t - (t + 1) // 2
        want["iters"][0, :t] = 1
        assert np.all(np.abs(c["resid"][0, :t] / (factor * tol) - 1.) < 1e-12)
        want["resid"][0, :t] = c["resid"][0, :t]
        expect_ctrl(c, want, raw)
        inert(ctx, kc.OP_DOT + kc.DOT_RR, [n + 3, n, t, 3], [tol],
              lambda active: [kc.fresh_ctrl(kc.rng_of(n, t, 3), t, active)[1], *dot_buffers(kc.DOT_RR, p, n)])
    print(f"dot rr: residual norm, worst error / tolerance {worst:.3g}")


@pytest.mark.parametrize("mode", range(4), ids=kc.DOT_NAMES)
def test_dot_marks_a_nan(ctx, mode):
    """a NaN at the last element of the last column: nan = 1 and PCG_ERROR off `active`, in every mode"""
    for case in kc.dot_cases():
        n, t = case["n"], case["t"]
        p = kc.dot_problem(mode, case)
        q = dict(a=p["a"].copy(), b=p["b"].copy())
        q["b" if mode in (kc.DOT_RZ, kc.DOT_PQ) else "a"][n - 1, t - 1] = np.nan
        a, b = dot_buffers(mode, q, n)
        active0 = 0 if mode == kc.DOT_BB else t
        c, raw = kc.fresh_ctrl(kc.rng_of(n, t, mode, 6), t, active0)
        was = c.copy()
        run(ctx, kc.OP_DOT + mode, [n + 3, n, t, 2], [kc.RR_TOL], [raw, a, b])
        others = t - 1 if mode == kc.DOT_BB else 0
        assert c["nan"][0] == 1 and c["npd"][0] == 0, case["id"]
        if mode == kc.DOT_RR:  # (the other columns may stop as well: every one of them takes at most 1 off)
            assert t - kc.PCG_ERROR - (t - 1) <= c["active"][0] <= t - kc.PCG_ERROR
        else:
            assert c["active"][0] == active0 + others - kc.PCG_ERROR, case["id"]
        for f in ("bb", "alpha", "beta", "resid", "iters", "stopped"):
            assert same_bits(c[f][0, t - 1:], was[f][0, t - 1:]), (case["id"], f)


def test_pcg_argument_checks(ctx):
    """an extent the kernel would address beyond a buffer: AGP_ERR_INVALID_ARGUMENT, nothing launched"""
    n, t = 65, 5
    rng = kc.rng_of(7)
    a = kc.padded(rng.standard_normal((n, t)), n + 3)[0]
    c, raw = kc.fresh_ctrl(rng, t, t)
    keep = raw.copy()
    short = a[:(n + 3) * (t - 1) + n - 1].copy()
    assert pcg_call(ctx, kc.OP_DOT + kc.DOT_RZ, [n + 3, n, t, 1], [1e-10], [raw, a, short]) == INVALID_ARGUMENT
    assert pcg_call(ctx, kc.OP_DOT + kc.DOT_RZ, [n - 1, n, t, 1], [1e-10], [raw, a, a.copy()]) == INVALID_ARGUMENT
    assert pcg_call(ctx, kc.OP_DOT + kc.DOT_RZ, [n + 3, n, 17, 1], [1e-10], [raw, a, a.copy()]) == INVALID_ARGUMENT
    assert pcg_call(ctx, kc.OP_DOT + kc.DOT_RZ, [n + 3, n, t, 1], [1e-10], [raw[:100].copy(), a, a.copy()]) == INVALID_ARGUMENT
    T1 = np.full(4 * t, np.nan)
    assert pcg_call(ctx, kc.OP_LT_R, [n + 3, n, 5, n + 3, t, 4], [], [raw, a, a.copy(), T1]) == INVALID_ARGUMENT  # ldt < m
    assert pcg_call(ctx, kc.OP_LT_R, [n + 3, n, 0, n + 3, t, 4], [], [raw, a, a.copy(), T1]) == INVALID_ARGUMENT  # m = 0: no grid
    assert pcg_call(ctx, kc.OP_PRECOND, [n + 3, n, 2, 4, n + 3, t], [0.5], [raw, a, None, a.copy(), a.copy()]) == INVALID_ARGUMENT
    assert pcg_call(ctx, kc.OP_SHIFT, [4, 5], [0.5], [np.zeros(25)]) == INVALID_ARGUMENT
    assert pcg_call(ctx, kc.OP_DIAG_STATS, [n], [], [np.ones(n), None, np.zeros(3)]) == INVALID_ARGUMENT
    assert pcg_call(ctx, kc.OP_VARIANCE + 1, [n], [], [np.ones(n)]) == INVALID_ARGUMENT
    assert same_bits(raw, keep)


# ---- pcg_lt_r_kernel ----------------------------------------------------------------------------------------------------------
def test_lt_r(ctx):
    worst, where = 0.0, None
    for case in kc.lt_r_cases():
        n, m, t = case["n"], case["m"], case["t"]
        p = kc.lt_r_problem(case)
        ldl, ldr, ldt = n + 3, n + 5, m + 2

        def make(active):
            return [kc.fresh_ctrl(kc.rng_of(n, m, t), t, active, stopped=(t - 1,))[1], kc.padded(p["L"], ldl)[0], kc.padded(p["R"], ldr)[0],
                    np.full(ldt * (t + 1) + 3, np.nan)]
        bufs = make(t)
        run(ctx, kc.OP_LT_R, [ldl, n, m, ldr, t, ldt], [], bufs, read_only=(0, 1, 2))
        T1 = bufs[3]
        ratio = kc.error_ratio(view(T1, ldt, m, t), p["ref"], p["bound"])
        assert ratio <= 1.0, (case["id"], ratio)
        if ratio >= worst:
            worst, where = ratio, case["id"]
        assert only_written(T1, np.full(len(T1), np.nan), ldt, m, t), case["id"]
        inert(ctx, kc.OP_LT_R, [ldl, n, m, ldr, t, ldt], [], make)
    print(f"lt_r: {len(kc.lt_r_cases())} cases, worst error / bound {worst:.3g} ({where})")


# ---- pcg_precond_kernel -------------------------------------------------------------------------------------------------------
def test_precond(ctx):
    worst, where = 0.0, None
    for case in kc.precond_cases():
        n, m, t = case["n"], case["m"], case["t"]
        p = kc.precond_problem(case)
        ldl, ldu, ld = n + 4, m + 2, n + 3
        for stopped in kc.stopped_sets(t):
            def make(active):
                return [kc.fresh_ctrl(kc.rng_of(n, m, t), t, active, stopped)[1], kc.padded(p["L"], ldl)[0] if m else None,
                        kc.padded(p["U"], ldu)[0] if m else None, kc.padded(p["R"], ld)[0], np.full(ld * (t + 1) + 3, np.nan)]
            bufs = make(t)
            run(ctx, kc.OP_PRECOND, [ldl, n, m, ldu, ld, t], [p["delta"]], bufs, read_only=(0, 1, 2, 3))
            Z = bufs[4]
            live = [k for k in range(t) if k not in stopped]
            got = view(Z, ld, n, t)[:, live]
            if m == 0:
                assert same_bits(got, np.ascontiguousarray((p["R"] / p["delta"])[:, live])), case["id"]
            ratio = kc.error_ratio(got, p["ref"][:, live], p["bound"][:, live]) if live else 0.0
            assert ratio <= 1.0, (case["id"], ratio)
            if ratio >= worst:
                worst, where = ratio, case["id"]
            assert only_written(Z, np.full(len(Z), np.nan), ld, n, t, skip_cols=stopped), case["id"]
            inert(ctx, kc.OP_PRECOND, [ldl, n, m, ldu, ld, t], [p["delta"]], make)
    print(f"precond: {len(kc.precond_cases())} cases, worst error / bound {worst:.3g} ({where})")


# ---- pcg_p_kernel, pcg_xr_kernel ----------------------------------------------------------------------------------------------
def sweep_ctrl(p, t, active, stopped):
    c, raw = kc.fresh_ctrl(kc.rng_of(t, 8), t, active, stopped)
    c["alpha"][0, :t], c["beta"][0, :t] = p["alpha"], p["beta"]
    return raw


def test_p(ctx):
    worst = 0.0
    for case in kc.sweep_cases():
        n, t = case["n"], case["t"]
        p = kc.sweep_problem(case)
        ld = n + 3
        for stopped in kc.stopped_sets(t):
            live = [k for k in range(t) if k not in stopped]
            for first in (1, 0):
                def make(active):
                    return [sweep_ctrl(p, t, active, stopped), kc.padded(p["Z"], ld)[0], kc.padded(p["P"], ld)[0]]
                bufs = make(t)
                before = bufs[2].copy()
                run(ctx, kc.OP_P, [ld, n, t, first], [], bufs, read_only=(0, 1))
                got = view(bufs[2], ld, n, t)[:, live]
                if first:
                    assert same_bits(got, np.ascontiguousarray(p["Z"][:, live])), case["id"]
                elif live:
                    ref, bound = kc.axpy_reference(p["Z"][:, live], p["beta"][live], p["P"][:, live])
                    ratio = kc.error_ratio(got, ref, bound)
                    assert ratio <= 1.0, (case["id"], ratio)
                    worst = max(worst, ratio)
                assert only_written(bufs[2], before, ld, n, t, skip_cols=stopped), case["id"]
                inert(ctx, kc.OP_P, [ld, n, t, first], [], make)
    print(f"p: {len(kc.sweep_cases())} cases, worst error / bound {worst:.3g}")


def test_xr(ctx):
    worst = 0.0
    for case in kc.sweep_cases():
        n, t = case["n"], case["t"]
        p = kc.sweep_problem(case)
        ldx, ld = n + 7, n + 3
        for stopped in kc.stopped_sets(t):
            live = [k for k in range(t) if k not in stopped]

            def make(active):
                return [sweep_ctrl(p, t, active, stopped), kc.padded(p["X"], ldx)[0], kc.padded(p["R"], ld)[0], kc.padded(p["P"], ld)[0],
                        kc.padded(p["Q"], ld)[0]]
            bufs = make(t)
            bx, br = bufs[1].copy(), bufs[2].copy()
            run(ctx, kc.OP_XR, [ldx, ld, n, t], [], bufs, read_only=(0, 3, 4))
            if live:
                for got, x, sign, v in ((view(bufs[1], ldx, n, t), p["X"], 1., p["P"]), (view(bufs[2], ld, n, t), p["R"], -1., p["Q"])):
                    ref, bound = kc.axpy_reference(x[:, live], sign * p["alpha"][live], v[:, live])
                    ratio = kc.error_ratio(got[:, live], ref, bound)
                    assert ratio <= 1.0, (case["id"], ratio)
                    worst = max(worst, ratio)
            assert only_written(bufs[1], bx, ldx, n, t, skip_cols=stopped) and only_written(bufs[2], br, ld, n, t, skip_cols=stopped), case["id"]
            inert(ctx, kc.OP_XR, [ldx, ld, n, t], [], make)
    print(f"xr: {len(kc.sweep_cases())} cases, worst error / bound {worst:.3g}")


# ---- pcg_diag_stats_kernel, pcg_shift_kernel, pcg_variance_kernel -------------------------------------------------------------
def test_diag_stats(ctx):
    worst = 0.0
    for case in kc.stats_cases():
        n = case["n"]
        p = kc.stats_problem(case)
        d, yv, stats = kc.vector(p["d"])[0], (kc.vector(p["yvar"])[0] if case["yvar"] else None), np.full(7, np.nan)
        run(ctx, kc.OP_DIAG_STATS, [n], [], [d, yv, stats], read_only=(0, 1))
        assert same_bits(stats[:2], np.array([p["max"], p["min"]])) and stats[3] == 0., (case["id"], stats, p["max"], p["min"])
        ratio = kc.error_ratio(stats[2:3], np.array([p["ref"]]), np.array([p["bound"]]))
        assert ratio <= 1.0, (case["id"], ratio)
        worst = max(worst, ratio)
        assert np.all(_bits(stats[4:]) == NAN_BITS)
        # a NaN at n - 1, in whichever input the case has last
        bad = kc.vector(p["yvar"] if case["yvar"] else p["d"])[0]
        bad[n - 1] = np.nan
        stats = np.full(7, np.nan)
        run(ctx, kc.OP_DIAG_STATS, [n], [], [d, bad, stats] if case["yvar"] else [bad, None, stats])
        assert stats[3] == 1. and np.all(_bits(stats[4:]) == NAN_BITS), case["id"]
    print(f"diag_stats: {len(kc.stats_cases())} cases, the sum's worst error / bound {worst:.3g}")


def test_shift(ctx):
    for m in kc.SHIFT_M:
        p = kc.shift_problem(m)
        ldc = m + 3
        flat = kc.padded(p["C"], ldc)[0]
        want = flat.copy()
        view(want, ldc, m, m)[:] = p["want"]
        run(ctx, kc.OP_SHIFT, [ldc, m], [p["delta"]], [flat])
        assert same_bits(flat, want), m
    print(f"shift: {len(kc.SHIFT_M)} sizes, bit for bit over the whole buffer")


def test_variance(ctx):
    worst = 0.0
    for case in kc.variance_cases():
        n, t = case["n"], case["t"]
        p = kc.variance_problem(case)
        ld = n + 3
        bufs = [kc.padded(p["Kc"], ld)[0], kc.padded(p["S"], ld)[0], kc.vector(p["prior"])[0], np.full(t + 3, np.nan)]
        run(ctx, kc.OP_VARIANCE, [ld, n, t], [], bufs, read_only=(0, 1, 2))
        ratio = kc.error_ratio(bufs[3][:t], p["ref"], p["bound"])
        assert ratio <= 1.0, (case["id"], ratio)
        worst = max(worst, ratio)
        assert np.all(_bits(bufs[3][t:]) == NAN_BITS)
    print(f"variance: {len(kc.variance_cases())} cases, worst error / bound {worst:.3g}")


# ---- the whole application on live fits ---------------------------------------------------------------------------------------
_SYSTEMS = {}


def system_of(ctx, name, with_var):
    """A = K + diag(y_var) from the device's Gram matrix, computed once"""
    key = (name, with_var)
    if key not in _SYSTEMS:
        cov, x, y, y_var = ic.inputs(name)
        _SYSTEMS[key] = ic.system(ctx.gram(cov, x), y_var if with_var else None)
    return _SYSTEMS[key]


def live_fit(ctx, name, with_var, rank):
    cov, x, y, y_var = ic.inputs(name)
    ds = ab.RegressionDataset(x, ab.MarginalDistribution(y, y_var) if with_var else y)
    model = ab.gp_from_covariance(cov, context=ctx)
    return model.fit_iterative(ds, preconditioner_rank=rank, preconditioner_tolerance=kc.PRECOND_REL_TOL, tolerance=ic.TOL).get_fit()


def download_state(ctx, fit):
    """agp_debug_iterative_state: (n, rank, delta, L (n x rank), the lower factor of delta I + L^T L (rank x rank))"""
    fn = capi.load_debug().agp_debug_iterative_state
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    dims, delta = np.full(3, -1, dtype=np.int64), np.full(1, np.nan)
    assert fn(ctx._h, fit._h, _p(dims), _p(delta), None, 0, None, 0) == 0
    n, m = int(dims[0]), int(dims[1])
    assert dims[2] >= n
    L = np.full((n + 3, max(m, 1)), np.nan, order="F")
    Cm = np.full((m + 1, max(m, 1)), np.nan, order="F")
    if m:
        assert fn(ctx._h, fit._h, _p(dims), _p(delta), _p(L), n + 3, _p(Cm), m + 1) == 0
        assert np.all(np.isnan(L[n:])) and np.all(np.isnan(Cm[m:])) and not np.isnan(L[:n]).any() and not np.isnan(Cm[:m]).any()
    return n, m, float(delta[0]), np.ascontiguousarray(L[:n, :m]), np.ascontiguousarray(Cm[:m, :m])


def precondition(ctx, fit, R, stopped):
    """agp_debug_iterative_precondition on padded host blocks: Z (n x t) and what came back around it"""
    fn = capi.load_debug().agp_debug_iterative_precondition
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
    n, t = R.shape
    Rb = np.full((n + 3, t), np.nan, order="F")
    Rb[:n] = R
    Zb = np.full((n + 5, t + 1), np.nan, order="F")
    marks = np.zeros(kc.PCG_COLS, dtype=np.int32)
    marks[list(stopped)] = 1
    keep = Rb.copy(order="F")
    assert fn(ctx._h, fit._h, _p(Rb), n + 3, t, _p(marks), _p(Zb), n + 5) == 0
    assert same_bits(Rb.ravel(order="F"), keep.ravel(order="F"))
    assert np.all(_bits(Zb[n:].ravel()) == NAN_BITS) and np.all(_bits(Zb[:, t].ravel()) == NAN_BITS)
    return Zb[:n, :t]


@pytest.mark.parametrize("case", kc.live_cases(), ids=lambda c: c["id"])
def test_application_on_live_fits(ctx, case):
    """delta, L and the factor a live fit holds, and one application of its preconditioner through the function every
    iteration calls, against longdouble from the downloaded L and delta.  The m = n cases (n65_3d rank 65, n2 rank 2) are in
    for their edges; their bound is about 1e-5 of max |Z| - the formula's own cancellation - and no evidence of accuracy."""
    name, rank, with_var = case["name"], case["rank"], case["with_var"]
    cov, x, y, y_var = ic.inputs(name)
    fit = live_fit(ctx, name, with_var, rank)
    n, m, delta, L, Cm = download_state(ctx, fit)
    assert (n, m) == (len(y), rank) and fit.preconditioner_rank == rank
    diag = np.diag(system_of(ctx, name, with_var)).copy()
    ref, bound = kc.delta_reference(diag, L)
    print(f"{case['id']}: delta {delta:.6g}, |delta - reference| / bound {abs(delta - ref) / bound:.3g}")
    assert abs(delta - ref) <= bound, (delta, ref, bound)
    if m == n:
        assert delta == ic.DELTA_FLOOR * diag.max()
    if not with_var:
        pub = ab.pivoted_cholesky(cov, ab.Measurement(x), rank, tolerance=kc.PRECOND_REL_TOL, context=ctx)
        assert pub.rank == rank and same_bits(L, np.ascontiguousarray(pub.factor)), "L is not the public pivoted Cholesky factor"
    app = kc.Application(L, delta)
    M, fb = app.factor_bound()
    ratio = kc.error_ratio(np.tril(Cm @ Cm.T), np.tril(M), np.tril(fb) + np.triu(np.ones((m, m)), 1))
    print(f"{case['id']}: the factor of delta I + L^T L, |C C^T - M| / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio
    for t in kc.LIVE_T:
        R = kc.live_rhs(n, t, m)
        stopped = kc.LIVE_STOPPED[t]
        live = [k for k in range(t) if k not in stopped]
        Z = precondition(ctx, fit, R, stopped)
        assert np.all(_bits(np.ascontiguousarray(Z[:, list(stopped)])) == NAN_BITS), "a stopped column was written"
        Zref, E = app.reference(R[:, live])
        ratio = kc.error_ratio(np.ascontiguousarray(Z[:, live]), Zref, E)
        print(f"{case['id']} t{t}: error / bound {ratio:.3g}; E / max|Z| {float(E.max() / np.abs(Zref).max()):.3g}")
        assert ratio <= 1.0, (case["id"], t, ratio)
    fit.close()


# ---- the columns of a chunk, through the public solve -------------------------------------------------------------------------
@pytest.mark.parametrize("rank", kc.INDEPENDENCE_RANKS)
def test_columns_of_a_chunk_are_independent(ctx, rank):
    """The column under test at position c of a 16-wide chunk has the same bits, iteration count and residual whether its
    neighbours are 15 copies of itself (all stop together), or a mix of columns that stop at least two looks of the host
    before it and columns that run at least two looks longer, in two different arrangements.  Only identical positions and
    chunk widths are compared.  tests/test_pcg_bounds_host.py shows the gaps in the float64 restatement."""
    A = system_of(ctx, kc.INDEPENDENCE_FIT, True)
    fit = live_fit(ctx, kc.INDEPENDENCE_FIT, True, rank)
    vs = kc.independence_vectors(A, rank)
    n = len(vs["test"])
    Xa, ia, ra = fit.solve(np.tile(vs["test"][:, None], (1, kc.PCG_COLS)), return_info=True)
    for c in kc.POSITIONS:
        for variant in (0, 1):
            B = kc.chunk_around(vs, c, variant)
            X, its, res = fit.solve(B, return_info=True)
            others = np.delete(its, c)
            print(f"rank {rank} position {c} arrangement {variant}: column under test {int(its[c])} iterations, neighbours {sorted({int(k) for k in others})}")
            assert others.min() + kc.DEVICE_GAP <= its[c] <= others.max() - kc.DEVICE_GAP, (its[c], others)
            assert its[c] == ia[c] and res[c] == ra[c], (c, variant, its[c], ia[c], res[c], ra[c])
            assert same_bits(X[:, c].copy(), Xa[:, c].copy()), (c, variant)
            for k in range(kc.PCG_COLS):  # a zero column: x = 0, no iteration, whatever runs beside it
                if not B[:, k].any():
                    assert its[k] == 0 and res[k] == 0. and not X[:, k].any()
    true = ic.true_residual(A, Xa[:, 0], vs["test"])
    assert true <= ic.residual_bound(A, Xa[:, 0], vs["test"]), true
    assert n == A.shape[0]
    fit.close()


@pytest.mark.parametrize("nrhs", [17, 33])
def test_columns_beyond_the_first_chunk(ctx, nrhs):
    """Columns 16 .. nrhs - 1 of a solve equal, bit for bit, the same vectors solved without the first 16 columns in front:
    column 16 is then column 0 of a chunk of the same width (17: a chunk of one; 33: a chunk of 16 and a chunk of one).  And
    the first 16 columns equal the same 16 solved alone.  No other pairing lands at the same position of a chunk of the
    same width, so no other is compared."""
    fit = live_fit(ctx, kc.INDEPENDENCE_FIT, True, 64)
    n = fit.n
    B = np.asfortranarray(kc.rng_of(n, nrhs, 20).standard_normal((n, nrhs)))
    X, its, res = fit.solve(B, return_info=True)
    Xt, it_t, res_t = fit.solve(B[:, 16:], return_info=True)
    Xh, it_h, res_h = fit.solve(B[:, :16], return_info=True)
    assert same_bits(np.ascontiguousarray(X[:, 16:]), np.ascontiguousarray(Xt)) and np.array_equal(its[16:], it_t)
    assert same_bits(res[16:].copy(), res_t)
    assert same_bits(np.ascontiguousarray(X[:, :16]), np.ascontiguousarray(Xh)) and np.array_equal(its[:16], it_h)
    assert same_bits(res[:16].copy(), res_h)
    print(f"nrhs {nrhs}: iterations {int(its.min())} .. {int(its.max())}")
    fit.close()
