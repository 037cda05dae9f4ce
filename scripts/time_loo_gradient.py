"""Exact gradient of the leave-one-out likelihood metric (leave_one_out_likelihood_gradient / agp_loo_nll_gradient)
against the tuner's forward differences of that metric: P + 1 value-only calls (LeaveOneOutLikelihood, one fit and
R = L^-1 each), the cost of compute_gradient (tune/finite_difference.hpp:37-90) on this objective.  Per stage of the
gradient call from the context's events (agp_last_stage_ms: 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 8 the
per-point terms, u and G, 9 G^T G, 7 contraction), and the G^T G kernel's rate (N^3 flop) against the fp64 MFMA peak
(78.6 TFLOP/s).

Workloads: config 3's problem (3-D SE(1, 1) + noise(0.1), P = 3) at N = 4096 and 16384; the temperature covariance
with explicit scale columns (bench.temperature_covariance, P = 6) at N = 16384.  Arguments: sizes of the config-3
workload (default 4096 16384)."""
import copy
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import albatross_amd as ab
import bench

ctx = ab.Context(0)
REPS = 5
STAGES = ((0, "gram"), (1, "factor"), (2, "alpha+R"), (6, "RtR"), (8, "terms+u+G"), (9, "GtG"), (7, "contraction"))


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
    metric = ab.LeaveOneOutLikelihood()
    steps = {k: 1e-6 * max(1., abs(v)) for k, v in base.items()}
    shifted = []
    for k, v in base.items():
        m = ab.gp_from_covariance_and_mean(copy.deepcopy(model.covariance_function_), copy.deepcopy(model.mean_function_),
                                           context=ctx)
        m.set_param_values({k: v + steps[k]})
        shifted.append(m)
    t_grad, (loo, grad) = timed(lambda: model.leave_one_out_likelihood_gradient(ds))
    ctx.set_profiling(True)
    model.leave_one_out_likelihood_gradient(ds)
    stages = {name: ctx.stage_ms(i) for i, name in STAGES}
    ctx.set_profiling(False)
    t_value, _ = timed(lambda: metric(ds, model))
    t_fwd, values = timed(lambda: [metric(ds, model)] + [metric(ds, m) for m in shifted])
    gtg_tflops = n ** 3 / (stages["GtG"] * 1e-3) / 1e12 if stages["GtG"] > 0 else float("nan")
    fd = {k: (values[i + 1] - values[0]) / steps[k] for i, k in enumerate(base)}
    print(f"{label}: N={n} P={P}")
    print(f"  leave_one_out_likelihood_gradient {t_grad:9.2f} ms   stages (events): "
          + ", ".join(f"{k} {v:.2f} ms" for k, v in stages.items()))
    print(f"  G^T G kernel: {gtg_tflops:.1f} TFLOP/s of N^3 flop ({gtg_tflops / 78.6:.2f} of 78.6)")
    print(f"  value only (LeaveOneOutLikelihood) {t_value:9.2f} ms")
    print(f"  P+1 = {P + 1:2d} value-only calls {t_fwd:9.2f} ms  ({t_fwd / t_grad:.2f} x the gradient call)")
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
