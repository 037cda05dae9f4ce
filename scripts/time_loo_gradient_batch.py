"""Batched leave-one-out likelihood and its exact gradient (agp_loo_nll_gradient_batch) at the sizes the reference's own
tuning example runs at (examples/sinc_example.cc: N = 256), against the loop a tuner would run instead:
  - the batched value + gradient (one call, B problems, 3 slots each, mean weights not asked for);
  - the batched value only (no slots: c_i from the column norms of R, no K^-1);
  - B sequential agp_loo_nll_gradient calls on the same problems (one launch chain per problem).
Model: 3-D SE(1, 1) + noise(0.1) with every parameter spread by +-20 % per problem.  Inputs are device-resident and the
C-ABI is called directly, so the times are those of the entries, not of the Python layer's model copies.  Wall-clock per
call after a warm-up, median of REPS.  Also the whole-batch device stage times of one profiled batched call
(agp_last_stage_ms: 0 gram, 1 factor, 2 alpha and R = L^-1, 6 R^T R, 8 per-point terms, u and G, 9 G^T G, 7 contraction).
Arguments: sizes (default 256 512 1024)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import albatross_amd as ab
import bench
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp

ctx = ab.Context(0)
lib = ctx._lib
REPS = 7
STAGES = ((0, "gram"), (1, "factor"), (2, "alpha+R"), (6, "RtR"), (8, "terms+u+G"), (9, "GtG"), (7, "contraction"))


def timed(fn):
    fn()
    ctx.synchronize()
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        times.append(time.perf_counter() - t)
    return statistics.median(times) * 1e3


def run(n, B):
    x, y = bench.make_dataset(n, 44)
    base = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1), context=ctx)
    rng = np.random.default_rng(n + B)
    sets = [{}] + [{k: v * (1. + 0.2 * rng.uniform(-1., 1.)) for k, v in base.get_params().items()} for _ in range(B - 1)]
    models = base._override_copies(sets)
    probs = [abgp._gradient_problem(m, ab.RegressionDataset(x, y)) for m in models]
    P = len(probs[0].slots)
    # only the coordinates move to the device and no tangent columns are passed: right for leaves without scale columns
    assert all(p.fs.scales is None and p.tangents is None for p in probs)
    coords = ctx.to_device(np.ravel(probs[0].fs.coords, order="K"))
    Y = ctx.to_device(np.ravel(np.asfortranarray(np.stack([p.y for p in probs], axis=1)), order="K"))
    structs = []
    for p in probs:
        s = p.fs.as_struct()
        s.coords = coords.ptr
        s.location = capi.DEVICE
        structs.append(s)
    handles = [ctx.private_kernel(m.covariance_function_) for m in models]
    kernels = (C.c_void_p * B)(*handles)
    fptrs = (C.c_void_p * B)(*[C.addressof(s) for s in structs])
    n_slots = (C.c_int * B)(*([P] * B))
    no_slots = (C.c_int * B)()
    tables = (C.c_void_p * B)(*[C.addressof(p.table) for p in probs])
    loo, grad, status = np.empty(B), np.empty((B, P)), (C.c_int * B)()
    only = np.empty(B)
    seq_loo, seq_grad = np.empty(B), np.empty((B, P))

    def batch():
        assert lib.agp_loo_nll_gradient_batch(ctx._h, B, kernels, fptrs, C.c_void_p(Y.ptr), n, None, 0, n_slots, tables, None, 0,
                                              C.c_void_p(loo.ctypes.data), C.c_void_p(grad.ctypes.data), P, None, 0, status) == 0

    def value_only():
        assert lib.agp_loo_nll_gradient_batch(ctx._h, B, kernels, fptrs, C.c_void_p(Y.ptr), n, None, 0, no_slots, None, None, 0,
                                              C.c_void_p(only.ctypes.data), None, 0, None, 0, status) == 0

    def loop():
        for b in range(B):
            v = C.c_double()
            assert lib.agp_loo_nll_gradient(ctx._h, handles[b], C.byref(structs[b]), C.c_void_p(Y.ptr + 8 * n * b), None, P,
                                            probs[b].table, None, 0, C.byref(v), C.c_void_p(seq_grad[b].ctypes.data), None) == 0
            seq_loo[b] = v.value

    t_batch, t_only, t_loop = timed(batch), timed(value_only), timed(loop)
    assert list(status) == [0] * B
    assert np.abs(loo - seq_loo).max() <= 1e-10 * np.abs(seq_loo).max() and np.abs(only - loo).max() <= 1e-12 * np.abs(loo).max()
    ctx.set_profiling(True)
    batch()
    stages = {name: ctx.stage_ms(i) for i, name in STAGES}
    ctx.set_profiling(False)
    print(f"N={n} B={B} P={P}: batch {t_batch:8.2f} ms | value only {t_only:8.2f} ms | loop of {B} single calls {t_loop:8.2f} ms "
          f"({t_loop / t_batch:.1f} x the batch) | {B / t_batch * 1e3:.0f} gradients/s")
    print(f"    device stages {sum(stages.values()):.2f} ms: " + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()), flush=True)
    for h in handles:
        lib.agp_kernel_destroy(h)
    coords.free()
    Y.free()


sizes = [int(a) for a in sys.argv[1:]] or [256, 512, 1024]
for n in sizes:
    for B in (8, 64, 256):
        run(n, B)
ctx.close()
