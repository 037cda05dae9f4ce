"""Predictions of B small fits: ONE agp_predict_batch call against the loop over agp_predict_mean / _marginal / _joint on
the same handles, in the same process (the loop is the code path users had before the batched entry existed).

Sizes: N in {512, 1024} training points, M in {64, 512} test points, B in {8, 32, 256} fits of one agp_fit_create_batch
call, all three modes.  Covariance: 3-D Matern-5/2 + independent noise with a different parameter vector per problem (one
tree: the one-launch path of the covariance kernels).  Outputs live in HBM (out_location = AGP_DEVICE); test features
live in HBM too (agp_features.location = AGP_DEVICE: launches and device work, no transfers) and, at N = 512, also in
pageable host memory, as the Python and C++ surfaces pass them (the uploads are part of both sides).  Per point:
3 warm-up calls, then the MEDIAN wall-clock time of REPS calls, batch and loop alternating, each call closed by its own
synchronisation; the loop's spread (min .. max of its REPS) is printed beside it as the run-to-run margin.  (The loop
passes 256 different covariance functions through the context's eight device-program slots, as any user's loop would.)
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


def test_features(m, B, where):
    """one feature vector per problem, resident in HBM or in pageable host memory"""
    rng = np.random.default_rng(m)
    keep, structs = [], []
    for b in range(B):
        a = np.ascontiguousarray(rng.uniform(0., 10., (m, 3)))
        d = ctx.to_device(a) if where == "device" else a
        f = capi.Features()
        f.n, f.dim, f.n_scale_columns, f.eq_id, f.scales, f.is_measurement = m, 3, 0, None, None, 0
        f.coords, f.location = (d.ptr, capi.DEVICE) if where == "device" else (a.ctypes.data, capi.HOST)
        keep.append(d)
        structs.append(f)
    return keep, structs


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


print(f"# median of {REPS} calls after {WARMUP} warm-up calls, ms; loop = B calls of agp_predict_* on the same handles")
print("| N | M | B | test features | mode | batch ms | loop ms (min .. max) | loop / batch |")
print("|---|---|---|---|---|---|---|---|")
for n in (512, 1024):
    for B in (8, 32, 256):
        models, fms = fit_problems(n, B)
        kernels = [ctx.private_kernel(m.covariance_function_) for m in models]
        karr = (C.c_void_p * B)(*kernels)
        farr = (C.c_void_p * B)(*[fm.get_fit()._h.value for fm in fms])
        # (host-resident test features - what the Python and C++ surfaces pass - at N = 512 only: they add the uploads)
        for m, where in [(m, w) for m in (64, 512) for w in (("device", "host") if n == 512 else ("device",))]:
            keep, structs = test_features(m, B, where)
            xarr = (C.c_void_p * B)(*[C.addressof(s) for s in structs])
            mean = ctx.device_empty(m * B)
            status = (C.c_int * B)()
            for mode, name in ((0, "mean"), (1, "marginal"), (2, "joint")):
                per = 0 if mode == 0 else (m if mode == 1 else m * m)
                second = ctx.device_empty(max(per, 1) * B)

                def batch():
                    rc = lib.agp_predict_batch(ctx._h, B, karr, farr, xarr, mode, C.c_void_p(mean.ptr), m, C.c_void_p(second.ptr), max(per, 1),
                                               capi.DEVICE, status)
                    assert rc == capi.AGP_OK

                def loop():
                    for b in range(B):
                        mp, sp = C.c_void_p(mean.ptr + 8 * m * b), C.c_void_p(second.ptr + 8 * per * b)
                        if mode == 0:
                            rc = lib.agp_predict_mean(ctx._h, kernels[b], farr[b], C.byref(structs[b]), mp, capi.DEVICE)
                        elif mode == 1:
                            rc = lib.agp_predict_marginal(ctx._h, kernels[b], farr[b], C.byref(structs[b]), mp, sp, capi.DEVICE)
                        else:
                            rc = lib.agp_predict_joint(ctx._h, kernels[b], farr[b], C.byref(structs[b]), mp, sp, capi.DEVICE)
                        assert rc == capi.AGP_OK

                tb, tl = times(batch, loop)
                mb, ml = statistics.median(tb), statistics.median(tl)
                print(f"| {n} | {m} | {B} | {where} | {name} | {mb:.3f} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {ml / mb:.1f} |", flush=True)
                del second
            del keep, mean
        for k in kernels:
            lib.agp_kernel_destroy(k)
        del fms
ctx.close()
