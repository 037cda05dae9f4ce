"""Times agp_pivoted_cholesky at (n, m) = (16384, 512), (65536, 1024), (262144, 2048): synthetic_3d features (bench.make_dataset)
with config 5's covariance, inputs resident on the device, L left on the device.  Per shape: ms of the call (best of
REPS after one warm-up), ms of the step chain alone (agp_last_stage_ms stage 10), the achieved read rate of L,
8 n rank^2 / 2 bytes / t, and beside it two references measured in the same run: the sparse GP fit of the same shape
(groups of 512, the pivots as inducing points; second call through the Python surface, host grouping included) and, at
(16384, 512) only, the float64 numpy restatement of tests/pivoted_chol_cases.py on the host.

    python scripts/time_pivoted_cholesky.py [shape index ...]
"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
from bench import make_dataset
import pivoted_chol_cases as pc

SHAPES = ((16384, 512), (65536, 1024), (262144, 2048))
REPS = 3
RESTATEMENT_AT = (16384, 512)

ctx = ab.Context(0)
shapes = tuple(SHAPES[int(a)] for a in sys.argv[1:]) or SHAPES
for n, m in shapes:
    x, y = make_dataset(n, 42)[:2]
    x = np.ascontiguousarray(x, dtype=np.float64)
    cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
    xd = ctx.to_device(x)
    s = capi.Features()
    s.n, s.dim, s.n_scale_columns = n, 3, 0
    s.coords, s.eq_id, s.scales = xd.ptr, None, None
    s.is_measurement, s.location = 0, capi.DEVICE
    Ld = ctx.device_empty((n * m,))
    rd = ctx.device_empty((n,))
    pivots = np.zeros(m, dtype=np.int64)
    rank, trace = C.c_int64(0), C.c_double(0.)
    kh = ctx.kernel(cov)

    def call():
        ctx._check(ctx._lib.agp_pivoted_cholesky(ctx._h, kh, C.byref(s), m, 0., C.c_void_p(pivots.ctypes.data), C.byref(rank),
                                                 C.c_void_p(Ld.ptr), n, C.c_void_p(rd.ptr), capi.DEVICE, C.byref(trace)),
                   "agp_pivoted_cholesky")

    call()
    ctx.set_profiling(True)
    best, chain = float("inf"), float("inf")
    for _ in range(REPS):
        t = time.perf_counter()
        call()
        best = min(best, time.perf_counter() - t)
        chain = min(chain, ctx.stage_ms(10))
    ctx.set_profiling(False)
    r = int(rank.value)
    read = 8. * n * r * r / 2.
    print(f"n={n} m={m}: rank {r}, call {best * 1e3:.2f} ms, step chain {chain:.2f} ms, L read rate "
          f"{read / (chain * 1e-3) / 1e12:.3f} TB/s ({read / 1e9:.2f} GB), trace residual {trace.value:.6g} of {n}")
    Ld.free()

    # reference 1: the sparse GP fit of the same shape with these inducing points
    u = x[pivots[:r]]

    def grouper(f):
        return np.arange(len(f)) // 512
    grouper.vectorized = True
    model = ab.sparse_gp_from_covariance(cov, grouper, ab.FixedInducingPoints(u), "pitc", context=ctx)
    model.set_param("inducing_nugget", 1e-6)
    ds = ab.RegressionDataset(x, np.asarray(y, dtype=np.float64))
    try:
        model.fit(ds)
        t = time.perf_counter()
        model.fit(ds)
        print(f"    sparse GP fit (PITC, groups of 512, m={r}): {(time.perf_counter() - t) * 1e3:.1f} ms")
    except ab.AlbatrossAmdError as e:
        print(f"    sparse GP fit: {e}")

    # reference 2: the float64 restatement on the host
    if (n, m) == RESTATEMENT_AT:
        kdiag = np.concatenate([np.diag(ctx.gram(cov, x[o:o + 2048])) for o in range(0, n, 2048)])

        def kcol(p):
            return ctx.gram(cov, x, x[p:p + 1])[:, 0]
        t = time.perf_counter()
        ref = pc.restatement(kdiag, kcol, m, 0.)
        print(f"    float64 numpy restatement on the host: {(time.perf_counter() - t) * 1e3:.0f} ms "
              f"(its columns of K come from the device; rank {ref[1]}, {int((ref[0] == pivots[:r]).sum())} of {r} pivots equal)")
    xd.free()
    rd.free()
ctx.close()
