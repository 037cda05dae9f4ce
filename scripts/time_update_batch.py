"""Updates of B small fits: ONE agp_fit_update_batch call against the loop over agp_fit_update on the same fits, in the
same process (the loop is the only route users had before the batched entry existed).

Shapes: N = 512 old points with m in {16, 64, 128} new ones for B in {8, 32, 256} fits of one agp_fit_create_batch
call, and N = 1024, m = 128, B = 64.  Covariance: 3-D Matern-5/2 + independent noise with a different parameter vector
per problem (one tree: the one-launch path of the covariance kernels).  New features, targets and variances live in HBM
(agp_features.location = AGP_DEVICE: launches and device work, no transfers).  Every call makes its fits and destroys
them again, so that both sides pay for their allocations as a streaming caller does.  Per point: 3 warm-up calls, then
the MEDIAN wall-clock time of REPS calls, batch and loop alternating; the loop's spread (min .. max of its REPS) is
printed beside it as the run-to-run margin.  A last profiled batch call gives the stage times of the context's stage
events: grow + cross covariance + V, Schur complement + factor, back substitution.
Arguments: REPS (default 20)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
WARMUP = 3
ctx = ab.Context(0)
lib = ctx._lib


def fit_problems(n, B):
    rng = np.random.default_rng(n + B)
    models, datasets = [], []
    for b in range(B):
        x = rng.uniform(0., 10., (n, 3))
        y = np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0])
        models.append(ab.gp_from_covariance(ab.Matern52(1.5 + 0.5 * b / B, 1.0) + ab.IndependentNoise(0.1 + 0.05 * b / B), context=ctx))
        datasets.append(ab.RegressionDataset(x, y))
    return models, ab.fit_batch(models, datasets)


def new_observations(m, B):
    """one feature vector per problem and the m x B targets and variances, all resident in HBM"""
    rng = np.random.default_rng(m)
    keep, structs = [], []
    for b in range(B):
        d = ctx.to_device(np.ascontiguousarray(rng.uniform(0., 10., (m, 3))))
        f = capi.Features()
        f.n, f.dim, f.n_scale_columns, f.eq_id, f.scales, f.is_measurement = m, 3, 0, None, None, 0
        f.coords, f.location = d.ptr, capi.DEVICE
        keep.append(d)
        structs.append(f)
    y = ctx.to_device(rng.standard_normal((B, m)))           # (column b of the m x B column-major matrix = row b here)
    v = ctx.to_device(rng.uniform(0.01, 0.05, (B, m)))
    return keep, structs, y, v


def times(first, second):
    """REPS timings (ms) of each of the two callables, alternating them so that both see the same machine"""
    for _ in range(WARMUP):
        first()
        second()
    a, b = [], []
    for _ in range(REPS):
        for fn, out in ((first, a), (second, b)):
            t = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t) * 1e3)
    return a, b


print(f"# median of {REPS} calls after {WARMUP} warm-up calls, ms; loop = B calls of agp_fit_update on the same fits; both destroy their fits")
print("| N | m | B | batch ms | loop ms (min .. max) | loop / batch | batch stages ms: grow+cross+V / Schur+factor / back substitution |")
print("|---|---|---|---|---|---|---|")
for n, shapes in ((512, [(m, B) for B in (8, 32, 256) for m in (16, 64, 128)]), (1024, [(128, 64)])):
    fitted = {}
    for m, B in shapes:
        if B not in fitted:
            fitted.clear()
            fitted[B] = fit_problems(n, B)
        models, fms = fitted[B]
        kernels = [ctx.private_kernel(mod.covariance_function_) for mod in models]
        karr = (C.c_void_p * B)(*kernels)
        farr = (C.c_void_p * B)(*[fm.get_fit()._h.value for fm in fms])
        keep, structs, y, v = new_observations(m, B)
        xarr = (C.c_void_p * B)(*[C.addressof(s) for s in structs])
        out = (C.c_void_p * B)()
        status = (C.c_int * B)()

        def batch():
            rc = lib.agp_fit_update_batch(ctx._h, B, karr, farr, xarr, C.c_void_p(y.ptr), m, C.c_void_p(v.ptr), m, out, None, 0, None, status)
            assert rc == capi.AGP_OK and not any(status)
            for b in range(B):
                lib.agp_fit_destroy(C.c_void_p(out[b]))

        def loop():
            handles = []
            for b in range(B):
                h = C.c_void_p()
                rc = lib.agp_fit_update(ctx._h, kernels[b], farr[b], C.byref(structs[b]), C.c_void_p(y.ptr + 8 * m * b),
                                        C.c_void_p(v.ptr + 8 * m * b), C.byref(h), None, None)
                assert rc == capi.AGP_OK
                handles.append(h)
            for h in handles:
                lib.agp_fit_destroy(h)

        tb, tl = times(batch, loop)
        ctx.set_profiling(True)
        batch()
        stages = " / ".join(f"{ctx.stage_ms(i):.3f}" for i in range(3))
        ctx.set_profiling(False)
        mb, ml = statistics.median(tb), statistics.median(tl)
        print(f"| {n} | {m} | {B} | {mb:.3f} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {ml / mb:.1f} | {stages} |", flush=True)
        for k in kernels:
            lib.agp_kernel_destroy(k)
        del keep, y, v
    fitted.clear()
ctx.close()
