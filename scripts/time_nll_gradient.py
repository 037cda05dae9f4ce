"""Exact gradient of the log-likelihood (log_likelihood_gradient / agp_nll_gradient) against the tuner's finite
differences: log_likelihoods() over P + 1 parameter sets (compute_gradient's forward difference,
tune/finite_difference.hpp:37-90) and over 2P + 1 sets (central differences).  Per stage of the gradient call from
the context's events (agp_last_stage_ms: 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 7 contraction), and the
R^T R kernel's rate against the fp64 MFMA peak (78.6 TFLOP/s).

Workloads: config 3's problem (3-D SE(1, 1) + noise(0.1), P = 3) at N = 4096 and 16384; the temperature covariance
with explicit scale columns (bench.temperature_covariance, P = 6) at N = 16384.  Arguments: sizes of the config-3
workload (default 4096 16384)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import albatross_amd as ab
import bench

ctx = ab.Context(0)
REPS = 5


def timed(fn):
    fn()
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(REPS):
        out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / REPS * 1e3, out


def run(label, model, ds):
    n = ds.size()
    base = model.get_params()
    P = len(base)
    fwd = [{}] + [{k: v + 1e-6 * max(1., abs(v))} for k, v in base.items()]
    cen = [{}] + [{k: v + s * 1e-6 * max(1., abs(v))} for k, v in base.items() for s in (1., -1.)]
    t_grad, (ll, grad) = timed(lambda: model.log_likelihood_gradient(ds))
    ctx.set_profiling(True)
    model.log_likelihood_gradient(ds)
    stages = {name: ctx.stage_ms(i) for i, name in ((0, "gram"), (1, "factor"), (2, "alpha+R"), (6, "RtR"), (7, "contraction"))}
    ctx.set_profiling(False)
    t_fwd, ll_fwd = timed(lambda: model.log_likelihoods(ds, fwd))
    t_cen, _ = timed(lambda: model.log_likelihoods(ds, cen))
    rtr_tflops = n ** 3 / 3. / (stages["RtR"] * 1e-3) / 1e12 if stages["RtR"] > 0 else float("nan")
    fd = {k: (ll_fwd[i + 1] - ll_fwd[0]) / (1e-6 * max(1., abs(base[k]))) for i, k in enumerate(base)}
    print(f"{label}: N={n} P={P}")
    print(f"  log_likelihood_gradient {t_grad:9.2f} ms   stages (events): "
          + ", ".join(f"{k} {v:.2f} ms" for k, v in stages.items()))
    print(f"  R^T R kernel: {rtr_tflops:.1f} TFLOP/s of N^3/3 flop ({100 * rtr_tflops / 78.6:.0f} % of 78.6)")
    print(f"  log_likelihoods P+1 = {P + 1:2d} sets {t_fwd:9.2f} ms  ({t_fwd / t_grad:.2f} x the gradient call)")
    print(f"  log_likelihoods 2P+1 = {2 * P + 1:2d} sets {t_cen:9.2f} ms  ({t_cen / t_grad:.2f} x the gradient call)")
    print("  max |forward difference - exact| / max|exact|: "
          f"{max(abs(fd[k] - grad[k]) for k in base) / max(abs(g) for g in grad.values()):.2e}", flush=True)


sizes = [int(a) for a in sys.argv[1:]] or [4096, 16384]
for n in sizes:
    x, y = bench.make_dataset(n, 44)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    run("config 3 (SE + noise)", model, ab.RegressionDataset(x, y))

n = 16384
ecef, h, temp = bench.synthetic_stations(n, 7)
cov, scale = bench.temperature_covariance(ab)
fs = ab.FeatureSet(ecef, [scale(h)])
model = ab.gp_from_covariance(cov, context=ctx)
run("temperature covariance, explicit scale column", model, ab.RegressionDataset(fs, temp - temp.mean()))
ctx.close()
