"""Batched exact gradients of the log-likelihood (log_likelihood_gradients / agp_nll_gradient_batch) at the sizes the
reference's users tune at, against the two things a tuner could do instead for the same B problems:
  - B sequential log_likelihood_gradient calls (agp_nll_gradient, one launch chain per problem);
  - log_likelihoods over B (P + 1) parameter sets (agp_nll_batch: batched forward differences, approximate).
Also one batched fit of the same B problems (fit_batch / agp_fit_create_batch) as the yardstick of the batch's factor,
the per-stage device times of one batched call (agp_last_stage_ms: 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R,
7 contraction) and the batched R^T R kernel's rate alone (agp_debug_rtr_lower_batched) against the fp64 MFMA peak.

Workloads: config 3's covariance (3-D SE(1, 1) + noise(0.1), P = 3) and the elevation-style ScalingTerm covariance
(ScalingTerm * Constant + Matern52 + noise, P = 6) at N = 512, 1024, 4096 with B = 1, 8, 64 (and 256 at N = 512).
Times are wall-clock per call through the Python surface (model copies and host assembly included), best of REPS.
Arguments: sizes (default 512 1024 4096)."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import albatross_amd as ab
import bench
from albatross_amd import _capi as capi

ctx = ab.Context(0)
REPS = 3
PEAK = 78.6  # fp64 MFMA TFLOP/s
FD_BYTES_MAX = 40e9  # skip the forward-difference batch whose slabs would exceed this


def timed(fn):
    out = fn()
    ctx.synchronize()
    best = float("inf")
    for _ in range(REPS):
        t = time.perf_counter()
        out = fn()
        ctx.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3, out


class Elevation(ab.ScalingFunction):
    _params = {"elevation_scaling_center": 4.0, "elevation_scaling_factor": 0.3}

    def get_name(self):
        return "elevation_scaling"

    def _call_impl(self, c):
        p = self.get_params()
        return 1. + p["elevation_scaling_factor"] * np.maximum(p["elevation_scaling_center"] - np.asarray(c)[:, 2], 0.)


def workloads():
    yield "config 3 (SE + noise)", lambda: ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1)
    yield "elevation ScalingTerm", lambda: ab.ScalingTerm(Elevation()) * ab.Constant(0.5) + ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1)


def parameter_sets(model, count, seed):
    rng = np.random.default_rng(seed)
    base = model.get_params()
    return [{}] + [{k: v * (1. + 0.2 * rng.uniform(-1., 1.)) for k, v in base.items()} for _ in range(count - 1)]


def rtr_rate(n, count):
    """the batched R^T R kernel alone: (ms, TFLOP/s of count N^3 / 3)"""
    dbg = capi.load_debug()
    dbg.agp_debug_rtr_lower_batched.restype = C.c_int
    dbg.agp_debug_rtr_lower_batched.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                C.POINTER(C.c_double)]
    R = np.zeros((count, n, n))
    for b in range(count):
        R[b] = np.triu(np.full((n, n), 1. / n)) + np.eye(n)  # column-major lower triangle
    out = np.zeros_like(R)
    ms = C.c_double()
    best = float("inf")
    for _ in range(REPS):
        assert dbg.agp_debug_rtr_lower_batched(ctx._h, C.c_void_p(R.ctypes.data), n, n, count, C.c_void_p(out.ctypes.data),
                                               C.byref(ms)) == 0
        best = min(best, ms.value)
    return best, count * n ** 3 / 3. / (best * 1e-3) / 1e12


def run(label, make, n, B):
    x, y = bench.make_dataset(n, 44)
    ds = ab.RegressionDataset(x, y)
    model = ab.gp_from_covariance(make(), context=ctx)
    P = len(model.get_params())
    sets = parameter_sets(model, B, n + B)
    copies = model._override_copies(sets)
    t_batch, (lls, grads) = timed(lambda: model.log_likelihood_gradients(ds, sets))
    t_seq, _ = timed(lambda: [m.log_likelihood_gradient(ds) for m in copies])
    fd_sets = []  # compute_gradient's forward difference at every problem's own parameters
    for m in copies:
        p = m.get_params()
        fd_sets += [dict(p)] + [dict(p, **{k: v + 1e-6 * max(1., abs(v))}) for k, v in p.items()]
    if len(fd_sets) * n * n * 8. <= FD_BYTES_MAX:
        t_fd, _ = timed(lambda: model.log_likelihoods(ds, fd_sets))
    else:
        t_fd = float("nan")
    t_fit, _ = timed(lambda: ab.fit_batch(copies, [ds] * B))
    ctx.set_profiling(True)
    model.log_likelihood_gradients(ds, sets)
    stages = {name: ctx.stage_ms(i) for i, name in ((0, "gram"), (1, "factor"), (2, "alpha+R"), (6, "RtR"), (7, "contraction"))}
    ctx.set_profiling(False)
    dev = sum(stages.values())
    print(f"{label}: N={n} B={B} P={P}")
    print(f"  batched gradient (one call)        {t_batch:9.2f} ms  ({t_batch / B:.3f} ms per problem)   device stages "
          f"{dev:.2f} ms: " + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()))
    print(f"  {B:3d} sequential gradient calls       {t_seq:9.2f} ms  ({t_seq / t_batch:.1f} x the batch)")
    if t_fd == t_fd:
        print(f"  log_likelihoods over B(P+1) = {len(fd_sets):4d}  {t_fd:9.2f} ms  ({t_fd / t_batch:.2f} x the batch)")
    else:
        print(f"  log_likelihoods over B(P+1) = {len(fd_sets):4d}  skipped (slabs > {FD_BYTES_MAX / 1e9:.0f} GB)")
    print(f"  fit_batch of the B problems        {t_fit:9.2f} ms  (batch = {t_batch / t_fit:.2f} x the fits)")
    if B * n * n <= 64 * 1024 * 1024:
        ms, tf = rtr_rate(n, B)
        print(f"  batched R^T R kernel alone: {ms:.3f} ms, {tf:.1f} TFLOP/s of B N^3/3 ({100 * tf / PEAK:.0f} % of {PEAK})")
    print(flush=True)


sizes = [int(a) for a in sys.argv[1:]] or [512, 1024, 4096]
for label, make in workloads():
    for n in sizes:
        for B in [1, 8, 64] + ([256] if n == 512 else []):
            run(label, make, n, B)
ctx.close()
