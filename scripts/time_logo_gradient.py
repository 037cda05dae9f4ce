"""Exact gradient of the leave-one-group-out likelihood metric (leave_one_group_out_likelihood_gradient /
agp_logo_nll_gradient) against agp_loo_nll_gradient at the same N, and the value-only call (LeaveOneGroupOutLikelihood)
against the same number from the host path that was there before it: cross_validate().scores(...) over the same groups
(one fit, held-out marginals, one metric call per group on the host; it scores marginals, so its number is the same
only for singleton groups - it is timed as the cost of that path, not compared).  Per stage of the gradient call from
the context's events (agp_last_stage_ms: 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 8 the group blocks, u and H,
9 the product C B C, 7 contraction), and the product's rate (N^3 flop) against the fp64 MFMA peak (78.6 TFLOP/s).

Workload: config 3's problem (3-D SE(1, 1) + noise(0.1), P = 3) with groups of 1, groups of 16 and ragged groups (sizes
1 ... 64 cycling through 1, 2, 3, 5, 8, 13, 21, 34, 64 over a random permutation).  Arguments: sizes (default 4096 16384)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import albatross_amd as ab
import bench

ctx = ab.Context(0)
REPS = 3
STAGES = ((0, "gram"), (1, "factor"), (2, "alpha+R"), (6, "RtR"), (8, "blocks+u+H"), (9, "CBC"), (7, "contraction"))
LOG_2PI = np.log(2 * np.pi)


def timed(fn, reps=REPS):
    fn()
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def groupings(n):
    perm = np.random.default_rng(n).permutation(n)
    ragged, at, k = {}, 0, 0
    sizes = (1, 2, 3, 5, 8, 13, 21, 34, 64)
    while at < n:
        m = min(sizes[k % len(sizes)], n - at)
        ragged[k] = perm[at:at + m].tolist()
        at += m
        k += 1
    return (("groups of 1", {i: [i] for i in range(n)}),
            ("groups of 16", {g: perm[16 * g:16 * g + 16].tolist() for g in range(n // 16)}),
            ("ragged 1..64", ragged))


def gaussian_nll(pred, truth):
    var = pred.covariance
    return float(np.sum(0.5 * (np.log(var) + (pred.mean - truth.mean) ** 2 / var + LOG_2PI)))


def run(n):
    x, y = bench.make_dataset(n, 44)
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    ds = ab.RegressionDataset(x, y)
    t_loo, _ = timed(lambda: model.leave_one_out_likelihood_gradient(ds))
    t_loo_value, _ = timed(lambda: ab.LeaveOneOutLikelihood()(ds, model))
    print(f"N={n}: agp_loo_nll_gradient {t_loo:9.2f} ms, value only {t_loo_value:9.2f} ms", flush=True)
    for label, indexer in groupings(n):
        metric = ab.LeaveOneGroupOutLikelihood(indexer)
        t_grad, (value, _) = timed(lambda: model.leave_one_group_out_likelihood_gradient(ds, indexer))
        ctx.set_profiling(True)
        model.leave_one_group_out_likelihood_gradient(ds, indexer)
        stages = {name: ctx.stage_ms(i) for i, name in STAGES}
        metric(ds, model)
        value_blocks = ctx.stage_ms(8)
        ctx.set_profiling(False)
        t_value, alone = timed(lambda: metric(ds, model))
        t_scores, _ = timed(lambda: model.cross_validate().scores(gaussian_nll, ds, indexer), reps=1)
        rate = n ** 3 / (stages["CBC"] * 1e-3) / 1e12 if stages["CBC"] > 0 else float("nan")
        print(f"  {label} ({len(indexer)} groups): value {value:.6f} (value-only call {alone:.6f})")
        print(f"    leave_one_group_out_likelihood_gradient {t_grad:9.2f} ms  ({t_grad / t_loo:.2f} x agp_loo_nll_gradient)   stages: "
              + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()))
        print(f"    C B C kernel: {rate:.1f} TFLOP/s of N^3 flop ({rate / 78.6:.2f} of 78.6)")
        print(f"    value only {t_value:9.2f} ms (group blocks {value_blocks:.2f} ms)   cross_validate().scores over the same groups "
              f"{t_scores:9.2f} ms  ({t_scores / t_value:.1f} x)", flush=True)


for n in [int(a) for a in sys.argv[1:]] or [4096, 16384]:
    run(n)
ctx.close()
