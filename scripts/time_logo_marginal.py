"""The Marginal predict type of the leave-one-group-out metric (agp_logo_nll_gradient_typed, AGP_PREDICT_MARGINAL):

1. value + gradient, Marginal against Joint (agp_logo_nll_gradient) at the same N and groups in the same process, the two
   alternating inside every repeat; per stage of the Marginal call from the context's events (agp_last_stage_ms: 0 gram,
   1 factor, 2 alpha and R = L^-1, 6 R^T R, 8 the group blocks, u and H, 9 the product C B C, 7 contraction);
2. the value-only call, with and without the per-group terms, against the way to the same numbers that was there before
   it: cross_validate().scores(gaussian_nll, ...) over the same groups (one fit, held-out marginals, one metric call per
   group on the host; the datasets here have no target variance, so both compute the same sum, which is printed).

Workload and groupings: those of scripts/time_logo_gradient.py (config 3's problem, 3-D SE(1, 1) + noise(0.1), P = 3;
groups of 1, groups of 16, ragged 1 ... 64).  Every call is warmed up once; a timed window is REPS calls that end in a
synchronise, the mean and the lowest and highest of ROUNDS windows are printed.  Arguments: sizes (default 4096 16384)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import albatross_amd as ab
import bench

ctx = ab.Context(0)
REPS, ROUNDS = 3, 3
STAGES = ((0, "gram"), (1, "factor"), (2, "alpha+R"), (6, "RtR"), (8, "blocks+u+H"), (9, "CBC"), (7, "contraction"))
LOG_2PI = np.log(2 * np.pi)


def window(fn, reps):
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def alternating(fns, reps=REPS, rounds=ROUNDS):
    """[(mean ms, lowest, highest, last result)] of the callables, each warmed up, their windows alternating"""
    for fn in fns:
        fn()
    times, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t, outs[i] = window(fn, reps)
            times[i].append(t)
    return [(float(np.mean(t)), min(t), max(t), o) for t, o in zip(times, outs)]


def show(t):
    return f"{t[0]:9.2f} ms [{t[1]:.2f} .. {t[2]:.2f}]"


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
    print(f"N={n}", flush=True)
    for label, indexer in groupings(n):
        marginal, joint = alternating([lambda: model.leave_one_group_out_likelihood_gradient(ds, indexer, predict_type="marginal"),
                                       lambda: model.leave_one_group_out_likelihood_gradient(ds, indexer)])
        ctx.set_profiling(True)
        model.leave_one_group_out_likelihood_gradient(ds, indexer, predict_type="marginal")
        stages = {name: ctx.stage_ms(i) for i, name in STAGES}
        model.leave_one_group_out_likelihood_gradient(ds, indexer)
        joint_blocks = ctx.stage_ms(8)
        ctx.set_profiling(False)
        metric = ab.LeaveOneGroupOutLikelihood(indexer, "marginal")
        value, terms = alternating([lambda: metric(ds, model), lambda: metric.group_scores(ds, model)])
        scores = alternating([lambda: model.cross_validate().scores(gaussian_nll, ds, indexer)], reps=1, rounds=2)[0]
        print(f"  {label} ({len(indexer)} groups): marginal value {marginal[3][0]:.6f} (value-only call {value[3]:.6f}, "
              f"sum of the host path's scores {float(np.sum(scores[3])):.6f}), joint value {joint[3][0]:.6f}")
        print(f"    value + gradient: marginal {show(marginal)}   joint {show(joint)}   marginal / joint {marginal[0] / joint[0]:.3f}")
        print("    marginal stages: " + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()) + f"   (joint blocks+u+H {joint_blocks:.2f})")
        print(f"    value only: {show(value)}   with the per-group terms {show(terms)}   cross_validate().scores {show(scores)}"
              f"  ({scores[0] / terms[0]:.1f} x the call with terms)", flush=True)


for n in [int(a) for a in sys.argv[1:]] or [4096, 16384]:
    run(n)
ctx.close()
