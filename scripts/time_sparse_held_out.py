"""agp_sparse_held_out (leave-one-group-out cross validation of the sparse model from one fit) against agp_sparse_nll and
agp_sparse_nll_gradient in the same process, with resident inputs (x, y, u in HBM) and the median of REPEATS calls after
one warm-up call: N = 65536 / m = 1024 and N = 262144 / m = 2048 (BASELINE config 5), groups of 512.  Then the cost of the
outputs (metric alone, Marginal, mean + variance, joint blocks left in HBM), the stages of one call (AGP_SPARSE_TIMING),
and at N = 65536 the only route there was before - fit(rest).predict(x_g).joint() - for 8 groups, extrapolated to all.
The table of DESIGN.md section 6g.  `time_sparse_held_out.py 0` runs the first size only."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import albatross_amd as ab
from albatross_amd import _capi as capi

REPEATS = 5
ctx = ab.Context(0)
lib = ctx._lib
CASES = ((65536, 1024, 512), (262144, 2048, 512))
if len(sys.argv) > 1:
    CASES = tuple(CASES[int(a)] for a in sys.argv[1:])


def median_ms(fn):
    fn()
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


for n, m, gs in CASES:
    rng = np.random.default_rng(n)
    x = np.sort(rng.uniform(0., n / 16., n))  # 1-D, ~16 points per unit length (scripts/time_sparse.py)
    y = np.sin(x) + 0.1 * np.cos(10. * x) + 0.1 * rng.standard_normal(n)
    yvar = rng.uniform(0.01, 0.04, n)  # (without target variances the Joint V_g of 512 close points is singular to working precision)
    cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
    u = np.linspace(x.min(), x.max(), m)
    offsets = np.arange(0, n + 1, gs, dtype=np.int64)
    G = len(offsets) - 1
    fx, fu = cov.features(x), cov.features(u)
    keep = [ctx.to_device(np.ravel(fx.coords)), ctx.to_device(np.ravel(fu.coords)), ctx.to_device(y), ctx.to_device(yvar)]
    sx, su = fx.as_struct(), fu.as_struct()
    sx.coords, sx.location = keep[0].ptr, capi.DEVICE
    su.coords, su.location = keep[1].ptr, capi.DEVICE
    yd, yv = C.c_void_p(keep[2].ptr), C.c_void_p(keep[3].ptr)
    kernel = ctx.kernel(cov)
    off = C.c_void_p(offsets.ctypes.data)
    slots, columns = cov.param_slots()
    assert not columns
    table = (capi.GradientSlot * len(slots))(*[capi.GradientSlot(node, p) for node, p, _ in slots])
    value, grad, nuggets = C.c_double(), np.zeros(len(slots)), np.zeros(2)
    mean_d, var_d = ctx.to_device(np.zeros(n)), ctx.to_device(np.zeros(n))
    joint_d = ab.gp.DeviceArray(ctx, 8 * n * gs)

    def nll():
        ctx._check(lib.agp_sparse_nll(ctx._h, kernel, C.byref(sx), G, off, yd, yv, C.byref(su), 1e-8, 1e-6, C.byref(value)), "agp_sparse_nll")

    def gradient():
        ctx._check(lib.agp_sparse_nll_gradient(ctx._h, kernel, C.byref(sx), G, off, yd, yv, C.byref(su), 1e-8, 1e-6, len(slots), table, None, n,
                                               None, m, C.byref(value), C.c_void_p(grad.ctypes.data), C.c_void_p(nuggets.ctypes.data), None),
                   "agp_sparse_nll_gradient")

    def held_out(ptype=capi.PREDICT_JOINT, mean=None, var=None, joint=None):
        def call():
            ctx._check(lib.agp_sparse_held_out(ctx._h, kernel, C.byref(sx), G, off, yd, yv, C.byref(su), 1e-8, 1e-6, ptype, C.byref(value),
                                               None, mean, var, joint), "agp_sparse_held_out")
        return call

    print(f"N={n} m={m} groups of {gs} ({G} groups), resident inputs, median (min .. max) of {REPEATS} calls in ms")
    rows = [("agp_sparse_nll", nll), ("agp_sparse_nll_gradient (%d slots)" % len(slots), gradient),
            ("agp_sparse_held_out, metric alone (Joint)", held_out()),
            ("agp_sparse_held_out, metric alone (Marginal)", held_out(capi.PREDICT_MARGINAL)),
            ("agp_sparse_held_out, metric + mean + variance", held_out(mean=C.c_void_p(mean_d.ptr), var=C.c_void_p(var_d.ptr))),
            ("agp_sparse_held_out, metric + joint blocks", held_out(joint=C.c_void_p(joint_d.ptr)))]
    for label, fn in rows:
        med, lo, hi = median_ms(fn)
        print(f"  {label:50s} {med:8.1f}  ({lo:.1f} .. {hi:.1f})   value {value.value:.6f}")
    os.environ["AGP_SPARSE_TIMING"] = "1"
    sys.stderr.flush()
    print("  stages of one metric-alone call (a synchronisation at every boundary):", flush=True)
    held_out()()
    print("  stages of one gradient call:", flush=True)
    gradient()
    del os.environ["AGP_SPARSE_TIMING"]
    if n == 65536:  # the only route before: one refit per group
        keys = np.arange(n) // gs
        sorted_x = x

        def grouper(f):
            return np.searchsorted(sorted_x, np.asarray(f, dtype=np.float64).reshape(-1)) // gs if np.ndim(f) else int(np.searchsorted(sorted_x, f) // gs)
        grouper.vectorized = True
        model = ab.sparse_gp_from_covariance(cov, grouper, ab.FixedInducingPoints(u), "pitc", context=ctx)
        model.set_param("inducing_nugget", 1e-6)
        times = []
        for g in range(0, G, G // 8)[:8]:
            rest = keys != g
            t = time.perf_counter()
            model.fit(ab.RegressionDataset(x[rest], ab.MarginalDistribution(y[rest], yvar[rest]))).predict(x[~rest]).joint()
            times.append((time.perf_counter() - t) * 1e3)
        med = statistics.median(times[1:])
        print(f"  fit(rest).predict(x_g).joint(), 8 groups: median {med:.1f} ms each -> {med * G / 1e3:.1f} s for all {G} groups")
        t = time.perf_counter()
        model.held_out_predictions(ab.RegressionDataset(x, ab.MarginalDistribution(y, yvar)))
        print(f"  model.held_out_predictions (host arrays, all groups): {(time.perf_counter() - t) * 1e3:.1f} ms")
    for d in keep + [mean_d, var_d, joint_d]:
        d.free()
