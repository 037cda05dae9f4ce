"""Times the probe gradient of the matrix-free fit: agp_gram_tangent_forms and agp_iterative_nll_gradient on synthetic_3d
features (bench.make_dataset) with config 5's covariance (three parameter slots), inputs resident on the device.  Every line
goes to stdout and to profiles/iterative_gradient/time_iterative_gradient.txt (--out PATH for another file).

  forms     n in (4096, 16384, 65536) x ncols in (1, 8, 16), P = 3: ms of the call (best of REPS after one warm-up) and
            pair-tangent evaluations per second (n (n + 1) / 2 pairs, each evaluated once for the three slots); at ncols = 16
            the time against 16 x the time of one column pair
  gradient  N = 16384 and 65536, t = 16 seeded probes, preconditioner ranks 256 and 1024: status, ms of the probe solves and
            of the forms (agp_last_stage_ms 12 / 13), wall ms, the worst probe's iterations, and the device memory in use
            after the call minus before it; beside agp_nll_gradient (the dense exact gradient) at the same N in the same run

    python scripts/time_iterative_gradient.py [forms] [gradient16384] [gradient65536] [--out PATH]
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

REPS = 3
TOL = 1e-10
PROBES = 16
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "iterative_gradient", "time_iterative_gradient.txt")
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
what = args or ["forms", "gradient16384", "gradient65536"]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
log = open(out_path, "w")


def say(line):
    print(line, flush=True)
    log.write(line + "\n")
    log.flush()


torch.cuda.init()  # torch's HIP runtime before the library's first HIP call (tests/conftest.py)
ctx = ab.Context(0)
cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
kh = ctx.kernel(cov)
slots = cov.param_slots()[0]
P = len(slots)
table = (capi.GradientSlot * P)(*[capi.GradientSlot(node, p) for node, p, _ in slots])
say(f"# {torch.cuda.get_device_name(0)}; slots {[nm for _, _, nm in slots]}")


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


if "forms" in what:
    say("# agp_gram_tangent_forms: n ncols ms pair_tangents_per_s  (t16 / (16 t1) in the ncols = 16 row)")
    for n in (4096, 16384, 65536):
        s, xd, yd = resident(n)
        t1 = None
        for ncols in (1, 8, 16):
            rng = np.random.default_rng(ncols)
            U, V = ctx.to_device(rng.standard_normal(n * ncols)), ctx.to_device(rng.standard_normal(n * ncols))
            forms = np.zeros((ncols, P), order="F")

            def call():
                ctx._check(ctx._lib.agp_gram_tangent_forms(ctx._h, kh, C.byref(s), P, table, None, n, C.c_void_p(U.ptr), n, C.c_void_p(V.ptr), n,
                                                           ncols, C.c_void_p(forms.ctypes.data), ncols, capi.DEVICE), "agp_gram_tangent_forms")
            t = best_of(call)
            t1 = t if ncols == 1 else t1
            tail = f"  t16/(16 t1) = {t / (16 * t1):.3f}" if ncols == 16 else ""
            say(f"forms n={n} ncols={ncols} P={P} ms={1e3 * t:.3f} pair_tangents_per_s={n * (n + 1) / 2 / t:.4g}{tail}")
            U.free()
            V.free()
        xd.free()
        yd.free()

MAX_ITERATIONS = 3000
for n in (16384, 65536):
    if f"gradient{n}" not in what:
        continue
    say(f"# gradient N = {n}, t = {PROBES} seeded probes, tolerance {TOL}")
    s, xd, yd = resident(n)
    ctx.set_profiling(True)
    for rep in range(2):  # the dense exact gradient: its first call pays for the workspace
        nll = C.c_double()
        grad = np.zeros(P)
        before = used_bytes()
        t = time.perf_counter()
        st = ctx._lib.agp_nll_gradient(ctx._h, kh, C.byref(s), C.c_void_p(yd.ptr), None, P, table, None, n, C.byref(nll),
                                       C.c_void_p(grad.ctypes.data), None)
        wall = time.perf_counter() - t
        say(f"dense_gradient N={n} call={rep} status={st} wall_ms={1e3 * wall:.1f} memory_delta_MB={(used_bytes() - before) / 1e6:.0f} "
            f"grad_nll={np.array2string(grad, precision=6)}")
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
        g, se = np.zeros(P), np.zeros(P)
        its, rs = np.zeros(PROBES, dtype=np.int32), np.zeros(PROBES)
        for rep in range(2):
            before = used_bytes()
            t = time.perf_counter()
            st = ctx._lib.agp_iterative_nll_gradient(ctx._h, h, P, table, None, n, PROBES, 1, None, 0, capi.DEVICE, C.c_void_p(g.ctypes.data),
                                                     C.c_void_p(se.ctypes.data), None, PROBES, C.c_void_p(its.ctypes.data),
                                                     C.c_void_p(rs.ctypes.data))
            wall = time.perf_counter() - t
            say(f"iterative_gradient N={n} rank={rank} call={rep} status={st} solves_ms={ctx.stage_ms(12):.1f} forms_ms={ctx.stage_ms(13):.1f} "
                f"wall_ms={1e3 * wall:.1f} worst_iterations={its.max()} memory_delta_MB={(used_bytes() - before) / 1e6:.0f} "
                f"grad_nll={np.array2string(g, precision=6)} stderr={np.array2string(se, precision=3)}")
        ctx._lib.agp_iterative_fit_destroy(h)
    ctx.set_profiling(False)
    xd.free()
    yd.free()
ctx.close()
log.close()
