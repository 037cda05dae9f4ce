"""Exact gradient of the sparse GP's log-likelihood (SparseGaussianProcessRegression.log_likelihood_gradient /
agp_sparse_nll_gradient) against the P + 1 evaluations of agp_sparse_nll that a forward-difference gradient costs
(tune/finite_difference.hpp:37-90), in one process, after warm-up, on random data: the benchmark's sparse workload
(bench.py config 5: 1-D, SE(1, 1) + measurement-only noise(0.1), uniformly spaced inducing points, groups of 512) at
N = 65536 / m = 1024 and N = 262144 / m = 2048.  P = 3 covariance parameters, 5 with the two nuggets.
With AGP_SPARSE_TIMING=1 in the environment the library prints the stage breakdown of every call on stderr (the fit's
stages, then the gradient's).  Arguments: "N:m" pairs (default 65536:1024 262144:2048)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import albatross_amd as ab

ctx = ab.Context(0)
REPS = 3


def timed(fn):
    fn()
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(REPS):
        out = fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / REPS * 1e3, out


def run(n, m, gs=512):
    rng = np.random.default_rng(n)
    x = np.sort(rng.uniform(0., n / 16., n))
    y = np.sin(x) + 0.1 * np.cos(10. * x) + 0.1 * rng.standard_normal(n)
    cov = ab.SquaredExponential(1.0, 1.0) + ab.measurement_only(ab.IndependentNoise(0.1))
    u = np.linspace(x.min(), x.max(), m)

    def grouper(f):
        return np.searchsorted(x, np.asarray(f, dtype=np.float64).reshape(-1)) // gs
    grouper.vectorized = True
    model = ab.sparse_gp_from_covariance(cov, grouper, ab.FixedInducingPoints(u), "pitc", context=ctx)
    model.set_param("inducing_nugget", 1e-6)
    ds = ab.RegressionDataset(x, y)
    t_nll, ll = timed(lambda: model.log_likelihood(ds))
    t_grad, (ll_g, grad) = timed(lambda: model.log_likelihood_gradient(ds))
    P = len(cov.get_params())
    added = 6. * n * m * m + 4. * n * gs * m + n * float(gs) ** 2  # flop of the gradient's solves and products beyond the fit
    print(f"sparse N={n} m={m} groups of {gs}: log_likelihood (a) {t_nll:8.2f} ms   log_likelihood_gradient (b) {t_grad:8.2f} ms")
    print(f"  (b) / (a) = {t_grad / t_nll:.2f};  (P + 1)(a) = {(P + 1) * t_nll:.1f} ms with P = {P}, {(P + 3) * t_nll:.1f} ms with the nuggets (P = {P + 2})")
    print(f"  work beyond the fit: {added:.3e} flop in {t_grad - t_nll:.1f} ms = {added / ((t_grad - t_nll) * 1e-3) / 1e12:.1f} TFLOP/s "
          f"(contractions included in the time)")
    print(f"  log p = {ll_g:.6f} (same as log_likelihood: {ll == ll_g});  gradient: " + ", ".join(f"{k} {v:.6e}" for k, v in grad.items()),
          flush=True)
    name, value = "squared_exponential_length_scale", cov.get_params()["squared_exponential_length_scale"]
    lls = []
    for v in (value + 1e-4, value - 1e-4):
        model.set_param(name, v)
        lls.append(model.log_likelihood(ds))
    model.set_param(name, value)
    fd = (lls[0] - lls[1]) / 2e-4
    print(f"  central difference of log_likelihood in {name}: {fd:.8e} (exact {grad[name]:.8e}, relative difference "
          f"{abs(fd - grad[name]) / abs(fd):.1e})", flush=True)
    if os.environ.get("AGP_SPARSE_TIMING"):
        print("  (one more gradient call for the stage breakdown on stderr)", flush=True)
        sys.stderr.write(f"--- stages, N={n} m={m} ---\n")
        sys.stderr.flush()
        model.log_likelihood_gradient(ds)


pairs = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(65536, 1024), (262144, 2048)]
for n, m in pairs:
    run(n, m)
ctx.close()
