"""Times the matrix-free fit: agp_gram_matvec, agp_iterative_fit_create and agp_iterative_predict_marginal on synthetic_3d
features (bench.make_dataset) with config 5's covariance, inputs resident on the device.

  matvec    n in (4096, 16384, 65536, 262144) x nrhs in (1, 8, 16): ms of the call (best of REPS after one warm-up), pair
            evaluations per second, and the time for 16 right-hand sides against 16 x the time for one
  fit       N = 16384 and 65536: agp_fit_create (dense fp64) and the iterative fit at preconditioner ranks 0, 256, 1024 in the
            same run; N = 262144: the iterative fit alone (no dense fit exists).  Per row: status, iterations, final relative
            residual, ms of the preconditioner build and of the conjugate-gradient chain (agp_last_stage_ms 11 / 12), wall ms,
            and the device memory in use after the call minus before it (hipMemGetInfo through torch; the cached scratch of
            the call is included, the peak inside the call is not visible this way)
  marginal  M test points at N = 65536 on the rank-1024 fit: ms, and ms per slice of 16

    python scripts/time_iterative_fit.py [matvec] [fit16384] [fit65536] [fit262144] [marginal16] [marginal256]
(no argument: matvec fit16384 fit65536 marginal16)
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

REPS = 3
TOL = 1e-10
MAX_ITERATIONS = {16384: 3000, 65536: 3000, 262144: 300}
what = sys.argv[1:] or ["matvec", "fit16384", "fit65536", "marginal16"]

torch.cuda.init()  # torch's HIP runtime before the library's first HIP call (tests/conftest.py)
ctx = ab.Context(0)
cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
kh = ctx.kernel(cov)


def used_bytes():
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def resident(n):
    x, y = make_dataset(n, 42)[:2]
    x = np.ascontiguousarray(x, dtype=np.float64)
    xd, yd = ctx.to_device(x), ctx.to_device(np.ascontiguousarray(y, dtype=np.float64))
    s = capi.Features()
    s.n, s.dim, s.n_scale_columns = n, 3, 0
    s.coords, s.eq_id, s.scales = xd.ptr, None, None
    s.is_measurement, s.location = 1, capi.DEVICE
    return s, xd, yd


def best_of(call):
    call()
    ctx.synchronize()
    best = float("inf")
    for _ in range(REPS):
        t = time.perf_counter()
        call()
        ctx.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


if "matvec" in what:
    print("# agp_gram_matvec: n nrhs ms pairs_per_s  (t16 / (16 t1) in the nrhs = 16 row)", flush=True)
    for n in (4096, 16384, 65536, 262144):
        s, xd, yd = resident(n)
        t1 = None
        for nrhs in (1, 8, 16):
            V = ctx.to_device(np.random.default_rng(nrhs).standard_normal(n * nrhs))
            out = ctx.device_empty((n * nrhs,))

            def call():
                ctx._check(ctx._lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, C.c_void_p(V.ptr), n, nrhs, C.c_void_p(out.ptr), n,
                                                    capi.DEVICE), "agp_gram_matvec")
            t = best_of(call)
            t1 = t if nrhs == 1 else t1
            tail = f"  t16/(16 t1) = {t / (16 * t1):.3f}" if nrhs == 16 else ""
            print(f"matvec n={n} nrhs={nrhs} ms={1e3 * t:.3f} pairs_per_s={n * n / t:.4g}{tail}", flush=True)
            V.free()
            out.free()
        xd.free()
        yd.free()


def iterative_fit(s, yd, n, rank):
    opt = capi.IterativeOptions(rank, 1e-12, TOL, MAX_ITERATIONS[n])
    h = C.c_void_p()
    it, res = C.c_int(0), C.c_double(0.)
    before = used_bytes()
    t = time.perf_counter()
    st = ctx._lib.agp_iterative_fit_create(ctx._h, kh, C.byref(s), C.c_void_p(yd.ptr), None, C.byref(opt), C.byref(h), None, C.byref(it),
                                           C.byref(res))
    wall = time.perf_counter() - t
    after = used_bytes()
    name = ctx._lib.agp_status_string(st).decode()
    got = int(ctx._lib.agp_iterative_fit_preconditioner_rank(h)) if h.value else -1
    print(f"iterative N={n} rank_asked={rank} rank={got} status='{name}' iterations={it.value} residual={res.value:.3e} "
          f"precond_ms={ctx.stage_ms(11):.1f} pcg_ms={ctx.stage_ms(12):.1f} wall_ms={1e3 * wall:.1f} "
          f"memory_delta_MB={(after - before) / 1e6:.0f}", flush=True)
    return h if h.value else None


for n in (16384, 65536, 262144):
    if f"fit{n}" not in what:
        continue
    print(f"# fit N = {n}", flush=True)
    s, xd, yd = resident(n)
    ctx.set_profiling(True)
    if n <= 65536:
        for rep in range(2):
            h = C.c_void_p()
            before = used_bytes()
            t = time.perf_counter()
            st = ctx._lib.agp_fit_create(ctx._h, kh, C.byref(s), C.c_void_p(yd.ptr), None, C.byref(h), None, None)
            wall = time.perf_counter() - t
            after = used_bytes()
            print(f"dense N={n} call={rep} status={st} wall_ms={1e3 * wall:.1f} memory_delta_MB={(after - before) / 1e6:.0f}", flush=True)
            if h.value:
                ctx._lib.agp_fit_destroy(h)
    for rank in ((0, 256, 1024) if n <= 65536 else (1024,)):
        h = iterative_fit(s, yd, n, rank)
        if h is not None:
            ctx._lib.agp_iterative_fit_destroy(h)
    ctx.set_profiling(False)
    xd.free()
    yd.free()

for m in (16, 256):
    if f"marginal{m}" not in what:
        continue
    n = 65536
    print(f"# marginal prediction, M = {m} at N = {n}, rank 1024", flush=True)
    s, xd, yd = resident(n)
    h = iterative_fit(s, yd, n, 1024)
    if h is None:
        print("marginal: no fit", flush=True)
        continue
    xs = np.random.default_rng(7).uniform(0., 10., (m, 3))
    fs = cov.features(xs)
    ss = fs.as_struct()
    mean, var = np.empty(m), np.empty(m)
    t = time.perf_counter()
    st = ctx._lib.agp_iterative_predict_marginal(ctx._h, kh, h, C.byref(ss), C.c_void_p(mean.ctypes.data), C.c_void_p(var.ctypes.data),
                                                 capi.HOST)
    wall = time.perf_counter() - t
    print(f"marginal M={m} status={st} ms={1e3 * wall:.1f} ms_per_16={1e3 * wall / -(-m // 16):.1f} "
          f"variance_min={var.min():.3e} variance_max={var.max():.3e}", flush=True)
    ctx._lib.agp_iterative_fit_destroy(h)
    xd.free()
    yd.free()
ctx.close()
