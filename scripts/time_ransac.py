"""GP RANSAC trial scoring (agp_ransac_score_trials) against the only route there was before it.

New call: one GPRansacScorer.score_raw over T trials (the whole call: uploads, Gram, gather, batched factor, scoring
launch, counts, download of the G x T metric matrix), wall clock around calls that end synchronised; per stage from the
context's events (agp_last_stage_ms: 0 gram, 2 gather, 1 factor, 8 scoring + counts).  The scoring stage is also printed
as the rate its gather traffic T * s * N * 8 bytes implies.

Old route: per trial model.fit(candidates' subset), then fit.predict(group).joint() for every held-out group and the
metric on the host.  That is G predictions per trial, so it is timed on ONE trial over a sample of at most 64 held-out
groups and EXTRAPOLATED linearly to G groups and T trials; the extrapolated figure is marked as such.

Shapes: N = 4096 and 16384 (3-D, Matern52(2, 1) + noise(0.1)); leave-one-out groups and groups of 16; samples of 3 and
8 groups; T = 64 and 1024.  Arguments: sizes (default 4096 16384)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import albatross_amd as ab
import bench

ctx = ab.Context(0)
LOG_2PI = np.log(2 * np.pi)
STAGES = ((0, "gram"), (2, "gather"), (1, "factor"), (8, "scoring"))


def timed(fn, reps=3):
    fn()
    best = []
    for _ in range(reps):
        ctx.synchronize()
        t = time.perf_counter()
        out = fn()
        ctx.synchronize()
        best.append((time.perf_counter() - t) * 1e3)
    return float(np.mean(best)), min(best), max(best), out


def old_route_ms(model, x, y, groups, candidates, sample=64):
    """one trial of the fit + predict(...).joint() loop over `sample` held-out groups, extrapolated to all of them"""
    chosen = set(candidates)
    pts = np.concatenate([groups[g] for g in candidates])
    held = [g for g in range(len(groups)) if g not in chosen][:sample]
    ctx.synchronize()
    t = time.perf_counter()
    fm = model.fit(ab.RegressionDataset(x[pts], y[pts]))
    fit_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    total = 0.
    for g in held:
        joint = fm.predict(ab.as_measurements(x[groups[g]])).joint()
        r = joint.mean - y[groups[g]]
        total += 0.5 * (np.linalg.slogdet(joint.covariance)[1] + r @ np.linalg.solve(joint.covariance, r) + len(r) * LOG_2PI)
    ctx.synchronize()
    per_group = (time.perf_counter() - t) * 1e3 / len(held)
    return fit_ms + per_group * (len(groups) - len(candidates)), fit_ms, per_group


def run(n):
    x, y = bench.make_dataset(n, 44)
    model = ab.gp_from_covariance(ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    ds = ab.RegressionDataset(x, y)
    print(f"N={n}", flush=True)
    for label, groups in (("groups of 1", [np.array([i]) for i in range(n)]),
                          ("groups of 16", [np.arange(a, a + 16) for a in range(0, n, 16)])):
        indexer = {k: g.tolist() for k, g in enumerate(groups)}
        strategy = ab.gp_ransac_strategy(ab.NegativeLogLikelihood("joint"), ab.FeatureCountConsensusMetric(), indexer)
        scorer = ab.GPRansacScorer(model, ds, strategy, 1.)
        for sample in (3, 8):
            s = sample * len(groups[0])
            old_trial, fit_ms, per_group = old_route_ms(model, x, y, groups, list(ab.draw_candidates(1, len(groups), sample, 1)[0]))
            old_trial2 = old_route_ms(model, x, y, groups, list(ab.draw_candidates(2, len(groups), sample, 1)[0]))[0]
            old_trial = min(old_trial, old_trial2)
            for T in (64, 1024):
                trials = ab.draw_candidates(0, len(groups), sample, T)
                new = timed(lambda: scorer.score_raw(trials))
                ctx.set_profiling(True)
                scorer.score_raw(trials)
                stages = {name: ctx.stage_ms(i) for i, name in STAGES}
                ctx.set_profiling(False)
                traffic = T * s * n * 8.
                rate = traffic / (stages["scoring"] * 1e-3) / 1e12 if stages["scoring"] > 0 else float("nan")
                old = old_trial * T
                print(f"  {label} ({len(groups)}), sample {sample} (s = {s}), T = {T}: new call {new[0]:9.2f} ms [{new[1]:.2f} .. {new[2]:.2f}]"
                      f"   stages " + ", ".join(f"{k} {v:.2f}" for k, v in stages.items())
                      + f"   scoring gather {traffic / 1e9:.2f} GB -> {rate:.3f} TB/s"
                      f"   old route (EXTRAPOLATED from one trial, {fit_ms:.2f} ms fit + {per_group:.3f} ms per group) {old:.0f} ms"
                      f"   ratio {old / new[0]:.0f} x", flush=True)


for n in [int(a) for a in sys.argv[1:]] or [4096, 16384]:
    run(n)
ctx.close()
