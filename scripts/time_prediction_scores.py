"""The prediction scores (include/albatross_amd.h, "scoring a joint prediction") on a joint covariance resident in HBM, at
m = 4096 and 16384 with the reference's 1000 samples: the time of each entry; for the L Z product of the draws its
fraction of the fp64 MFMA peak (m^2 k flop, 78.6 TFLOP/s); for the variogram pass its fraction of the HBM roofline (the
bytes of one triangle, 8.0 TB/s); beside them download + numpy of the same quantities on this host.

    python scripts/time_prediction_scores.py [m ...]
"""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import albatross_amd as ab
from albatross_amd import _capi as capi

PEAK_FP64, PEAK_HBM = 78.6e12, 8.0e12
SAMPLES, SEED = 1000, 22
K = SAMPLES // 2 + 1


def best(call, repeats=3):
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return min(ts)


ctx = ab.Context(0)
lib = ctx._lib
covariance = ab.SquaredExponential(2.0, 1.0) + ab.IndependentNoise(0.3)
kh = ctx.kernel(covariance)
for m in [int(a) for a in sys.argv[1:]] or [4096, 16384]:
    rng = np.random.default_rng(m)
    x = rng.uniform(0., 10., (m, 3))
    features = covariance.features(x)
    feats = features.as_struct()
    cov_d = ctx.device_empty((m, m))
    assert lib.agp_gram(ctx._h, kh, C.byref(feats), None, C.c_void_p(cov_d.ptr), m, capi.DEVICE) == 0
    mean, truth = rng.standard_normal(m), rng.standard_normal(m)
    mean_d, truth_d = ctx.to_device(mean), ctx.to_device(truth)
    out = C.c_double()
    P = lambda d: C.c_void_p(d.ptr)  # noqa: E731

    # --- device ---------------------------------------------------------------------------------------------------------
    h = C.c_void_p()
    t_factor = best(lambda: (h.value and lib.agp_fit_destroy(h), lib.agp_factor_create(ctx._h, P(cov_d), m, m, 0, capi.DEVICE, C.byref(h))), 2)
    z_d, s_d = ctx.device_empty((m, 2 * K)), ctx.device_empty((m, 2 * K))
    t_normal = best(lambda: lib.agp_standard_normal(ctx._h, SEED, m, 0, 2 * K, P(z_d), m, capi.DEVICE))
    t_draw = best(lambda: lib.agp_draw_mvn(ctx._h, h, P(mean_d), 2 * K, SEED, P(z_d), m, P(s_d), m, capi.DEVICE))
    t_draw_gen = best(lambda: lib.agp_draw_mvn(ctx._h, h, P(mean_d), 2 * K, SEED, None, 0, P(s_d), m, capi.DEVICE))
    t_energy = best(lambda: lib.agp_energy_score(ctx._h, P(mean_d), P(cov_d), m, m, P(truth_d), None, None, SEED, SAMPLES, None, 0,
                                                capi.DEVICE, C.byref(out)), 2)
    es = out.value
    t_vario = {}
    vs = {}
    for order in (1, 2):
        t_vario[order] = best(lambda: lib.agp_variogram_score(ctx._h, P(mean_d), P(cov_d), m, m, P(truth_d), None, None, 0, order,
                                                              capi.DEVICE, C.byref(out)))
        vs[order] = out.value
    sig_d, crps_d = ctx.to_device(rng.uniform(0.1, 2., m)), ctx.device_empty(m)
    t_crps = best(lambda: lib.agp_crps_normal(ctx._h, P(mean_d), P(sig_d), P(truth_d), m, P(crps_d), capi.DEVICE))
    lib.agp_fit_destroy(h)
    flop, tri_bytes = float(m) * m * 2 * K, 8. * m * (m + 1) / 2
    print(f"m={m} k={K}: factor {1e3 * t_factor:.2f} ms | normals (m x 2k) {1e3 * t_normal:.2f} ms | "
          f"draw L Z, z supplied {1e3 * t_draw:.2f} ms = {flop / t_draw / 1e12:.1f} TFLOP/s = {flop / t_draw / PEAK_FP64:.2f} of the fp64 MFMA peak"
          f" (with the generator {1e3 * t_draw_gen:.2f} ms) | energy score {1e3 * t_energy:.2f} ms ({es:.6e})", flush=True)
    for order in (1, 2):
        print(f"m={m}: variogram order {order} {1e3 * t_vario[order]:.3f} ms = {tri_bytes / t_vario[order] / 1e12:.2f} TB/s = "
              f"{tri_bytes / t_vario[order] / PEAK_HBM:.2f} of the HBM roofline ({vs[order]:.6e}) | crps ({m}) {1e3 * t_crps:.3f} ms", flush=True)

    # --- download + numpy on this host --------------------------------------------------------------------------------------
    t0 = time.perf_counter()
    cov = cov_d.numpy()
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    L = np.linalg.cholesky(cov)
    t_chol = time.perf_counter() - t0
    t0 = time.perf_counter()
    v = L @ np.random.default_rng(SEED).standard_normal((m, 2 * K))
    t_gemm = time.perf_counter() - t0
    t0 = time.perf_counter()
    d = np.diag(cov)
    total = 0.
    for row in range(m - 1):  # order 2: no erf on the host side either
        s2 = d[row] + d[row + 1:] - 2. * cov[row, row + 1:]
        diff = (truth[row] - truth[row + 1:]) ** 2 - ((mean[row + 1:] - mean[row]) ** 2 + s2)
        total += (diff * diff).sum()
    t_np_vario = time.perf_counter() - t0
    print(f"m={m}: host: download {1e3 * t_down:.1f} ms, numpy cholesky {1e3 * t_chol:.1f} ms, L @ Z {1e3 * t_gemm:.1f} ms, "
          f"variogram order 2 {1e3 * t_np_vario:.1f} ms ({total:.6e}); sample checksum {float(np.abs(v).sum()):.6e}", flush=True)
