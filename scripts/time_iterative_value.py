"""Times the log-likelihood value of the matrix-free fit (agp_iterative_nll) on synthetic_3d features (bench.make_dataset)
with config 5's covariance (three parameter slots), inputs resident on the device - the setup of
scripts/time_iterative_gradient.py.  Every line goes to stdout and to profiles/iterative_value/time_iterative_value.txt
(--out PATH for another file).

  N = 16384 and 65536, t = 16 seeded probes, preconditioner ranks 256 and 1024, in one run per N:
    value      agp_iterative_nll with n_slots = 0: wall ms, ms of the probe solves / the probes, quadrature and log det P
               (agp_last_stage_ms 12 / 14), the value, its standard error, the worst probe's iterations
    combined   agp_iterative_nll with the three slots: wall ms, stages 12 / 13 / 14, value and gradient
    gradient   agp_iterative_nll_gradient (Rademacher probes): wall ms, stages 12 / 13
    ratio      combined / (value + gradient), wall
    solve      agp_iterative_solve on the SAME 16 probes (downloaded from the probe kernel's entry, resident on the device):
               wall ms and ms per iteration, beside the value call's stage 12 per iteration (the record launch included)
    quadrature the host quadrature alone on the 16 logged coefficient sets (agp_debug_lanczos_quadrature), ms
  N = 16384 also: the dense value (agp_nll) and the distance of the estimate from it in standard errors.

    python scripts/time_iterative_value.py [value16384] [value65536] [--out PATH]
(no argument: everything)
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import albatross_amd as ab
from albatross_amd import _capi as capi
from bench import make_dataset

TOL = 1e-10
PROBES = 16
SEED = 1
MAX_ITERATIONS = 3000
COLS = 16  # PCG_COLS
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "iterative_value", "time_iterative_value.txt")
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
what = args or ["value16384", "value65536"]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
log = open(out_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


def P_(a):
    return C.c_void_p(a.ctypes.data)


torch.cuda.init()  # torch's HIP runtime before the library's first HIP call (tests/conftest.py)
ctx = ab.Context(0)
cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
kh = ctx.kernel(cov)
slots = cov.param_slots()[0]
P = len(slots)
table = (capi.GradientSlot * P)(*[capi.GradientSlot(node, p) for node, p, _ in slots])
dbg = capi.load_debug()
say(f"# {torch.cuda.get_device_name(0)}; slots {[nm for _, _, nm in slots]}; t = {PROBES}, seed {SEED}, tolerance {TOL}")


def resident(n):
    x, y = make_dataset(n, 42)[:2]
    x = np.ascontiguousarray(x, dtype=np.float64)
    xd, yd = ctx.to_device(x), ctx.to_device(np.ascontiguousarray(y, dtype=np.float64))
    s = capi.Features()
    s.n, s.dim, s.n_scale_columns = n, 3, 0
    s.coords, s.eq_id, s.scales = xd.ptr, None, None
    s.is_measurement, s.location = 1, capi.DEVICE
    return s, xd, yd


def value_call(h, n, with_gradient):
    """(status, wall ms, nll, stderr, log det, grad, grad stderr, iterations) of one agp_iterative_nll call"""
    nll, se, ld = C.c_double(), C.c_double(), C.c_double()
    g, gse = np.zeros(P), np.zeros(P)
    its = np.zeros(PROBES, dtype=np.int32)
    t = time.perf_counter()
    st = ctx._lib.agp_iterative_nll(ctx._h, h, PROBES, SEED, None, 0, capi.DEVICE, 0., P if with_gradient else 0,
                                    table if with_gradient else None, None, n, C.byref(nll), C.byref(se), C.byref(ld), None,
                                    P_(g) if with_gradient else None, P_(gse) if with_gradient else None, None, PROBES, P_(its), None)
    return st, 1e3 * (time.perf_counter() - t), nll.value, se.value, ld.value, g, gse, its


for n in (16384, 65536):
    if f"value{n}" not in what:
        continue
    say(f"# N = {n}")
    reps = 2 if n <= 16384 else 1  # (a second call repeats the first to the millisecond: profiles/iterative_gradient)
    s, xd, yd = resident(n)
    ctx.set_profiling(True)
    dense = None
    if n == 16384:
        out = C.c_double()
        for rep in range(2):
            t = time.perf_counter()
            st = ctx._lib.agp_nll(ctx._h, kh, C.byref(s), C.c_void_p(yd.ptr), None, C.byref(out))
            say(f"dense_value N={n} call={rep} status={st} wall_ms={1e3 * (time.perf_counter() - t):.1f} nll={out.value:.6f}")
        dense = out.value
    for rank in (256, 1024):
        opt = capi.IterativeOptions(rank, 1e-12, TOL, MAX_ITERATIONS)
        h = C.c_void_p()
        it, res = C.c_int(0), C.c_double(0.)
        t = time.perf_counter()
        st = ctx._lib.agp_iterative_fit_create(ctx._h, kh, C.byref(s), C.c_void_p(yd.ptr), None, C.byref(opt), C.byref(h), None, C.byref(it),
                                               C.byref(res))
        say(f"iterative_fit N={n} rank={rank} status={st} iterations={it.value} wall_ms={1e3 * (time.perf_counter() - t):.1f}")
        if not h.value:
            continue
        walls = {}
        for rep in range(reps):
            st, wall, nll, se, ld, _, _, its = value_call(h, n, False)
            walls["value"] = wall
            solves_value, iters_value = ctx.stage_ms(12), int(its.max())
            tail = f" dense_nll={dense:.6f} standard_errors_from_dense={abs(nll - dense) / se:.2f}" if dense is not None else ""
            say(f"value N={n} rank={rank} call={rep} status={st} wall_ms={wall:.1f} solves_ms={ctx.stage_ms(12):.1f} "
                f"probes_quadrature_logdetP_ms={ctx.stage_ms(14):.2f} nll={nll:.6f} stderr={se:.4g} log_det={ld:.6f} "
                f"worst_iterations={its.max()}{tail}")
        for rep in range(reps):
            st, wall, nll, se, ld, g, gse, its = value_call(h, n, True)
            walls["combined"] = wall
            say(f"combined N={n} rank={rank} call={rep} status={st} wall_ms={wall:.1f} solves_ms={ctx.stage_ms(12):.1f} "
                f"forms_ms={ctx.stage_ms(13):.1f} probes_quadrature_logdetP_ms={ctx.stage_ms(14):.2f} nll={nll:.6f} stderr={se:.4g} "
                f"grad_nll={np.array2string(g, precision=6)} grad_stderr={np.array2string(gse, precision=3)}")
        g, gse = np.zeros(P), np.zeros(P)
        its = np.zeros(PROBES, dtype=np.int32)
        for rep in range(reps):
            t = time.perf_counter()
            st = ctx._lib.agp_iterative_nll_gradient(ctx._h, h, P, table, None, n, PROBES, SEED, None, 0, capi.DEVICE, P_(g), P_(gse), None,
                                                     PROBES, P_(its), None)
            walls["gradient"] = 1e3 * (time.perf_counter() - t)
            say(f"gradient N={n} rank={rank} call={rep} status={st} wall_ms={walls['gradient']:.1f} solves_ms={ctx.stage_ms(12):.1f} "
                f"forms_ms={ctx.stage_ms(13):.1f} worst_iterations={its.max()} grad_nll={np.array2string(g, precision=6)} "
                f"grad_stderr={np.array2string(gse, precision=3)}")
        say(f"ratio N={n} rank={rank} combined/(value+gradient)={walls['combined'] / (walls['value'] + walls['gradient']):.3f}")
        # the same 16 probes through agp_iterative_solve (no record launch), resident on the device
        dbg.agp_debug_iterative_probes.restype = C.c_int
        dbg.agp_debug_iterative_probes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p, C.c_int64]
        Z = np.empty((n, PROBES), order="F")
        assert dbg.agp_debug_iterative_probes(ctx._h, h, SEED, PROBES, P_(Z), n) == 0
        Zd, Xd = ctx.to_device(np.ascontiguousarray(Z.T)), ctx.device_empty((n, PROBES))
        its = np.zeros(PROBES, dtype=np.int32)
        ctx.set_profiling(False)
        for rep in range(reps):
            t = time.perf_counter()
            st = ctx._lib.agp_iterative_solve(ctx._h, h, C.c_void_p(Zd.ptr), n, PROBES, C.c_void_p(Xd.ptr), n, capi.DEVICE, P_(its), None)
            wall = 1e3 * (time.perf_counter() - t)
            say(f"solve N={n} rank={rank} call={rep} status={st} wall_ms={wall:.1f} worst_iterations={its.max()} "
                f"ms_per_iteration={wall / max(1, its.max()):.4f}  value_call_solves_ms_per_iteration={solves_value / max(1, iters_value):.4f}")
        ctx.set_profiling(True)
        Zd.free()
        Xd.free()
        # the host quadrature alone, on the coefficients of the same probes
        fn = dbg.agp_debug_iterative_solve_logged
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_int64, C.c_double, C.c_void_p]
        mi = C.c_int(0)
        X = np.empty((n, PROBES), order="F")
        lg = np.zeros(COLS * (1 + 2 * MAX_ITERATIONS))
        its = np.zeros(PROBES, dtype=np.int32)
        st = fn(ctx._h, h, P_(Z), n, PROBES, P_(X), n, P_(its), None, P_(lg), lg.size, 0., C.byref(mi))
        assert st == 0 and mi.value == MAX_ITERATIONS
        al = lg[COLS:COLS + COLS * MAX_ITERATIONS].reshape(MAX_ITERATIONS, COLS)
        be = lg[COLS + COLS * MAX_ITERATIONS:].reshape(MAX_ITERATIONS, COLS)
        q = dbg.agp_debug_lanczos_quadrature
        q.restype = C.c_int
        q.argtypes = [C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        cols = [(float(lg[c]), np.ascontiguousarray(al[:its[c], c]), np.ascontiguousarray(be[:its[c], c])) for c in range(PROBES)]
        out = np.zeros(1)
        t = time.perf_counter()
        for rz0, a, b in cols:
            assert q(rz0, P_(a), P_(b), len(a), P_(out)) == 0
        say(f"quadrature N={n} rank={rank} columns={PROBES} rows={its.min()}..{its.max()} host_ms={1e3 * (time.perf_counter() - t):.2f}")
        ctx._lib.agp_iterative_fit_destroy(h)
    ctx.set_profiling(False)
    xd.free()
    yd.free()
ctx.close()
log.close()
