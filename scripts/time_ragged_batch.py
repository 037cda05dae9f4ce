"""Fit, predict and update B small fits of UNEQUAL sizes: the ragged batched entries (one agp_fit_create_batch_ragged /
agp_predict_batch / agp_fit_update_batch call per size class ceil(n_b / 128), as ab.fit_batch / predict_batch /
update_batch make them) against
  (a) the loop over agp_fit_create / agp_predict_* / agp_fit_update on the same problems in the same process - the only
      route a caller with unequal sizes had before - and
  (b) ONE equal-size batch of B fits that all have the largest size of the draw: what the split into classes and the
      padding cost against a batch that needs neither.

Shapes: B in {8, 32, 256} fits with sizes drawn uniformly from 129..512 and from 400..512 (seeded), M = 128 test points
per problem, m = 64 new observations per problem.  Covariance: 3-D Matern-5/2 + independent noise with a different
parameter vector per problem (one tree: the one-launch path of the covariance kernels).  Every input lives in HBM
(agp_features.location = AGP_DEVICE: launches and device work, no transfers) and the predictions stay there.  The fit and
update calls make their fits and destroy them again, so that every side pays for its allocations as a streaming caller
does.  Per point: 3 warm-up calls, then the MEDIAN wall-clock time of REPS calls, the three sides alternating; the loop's
spread (min .. max of its REPS) is printed beside it as the run-to-run margin.
Arguments: REPS (default 20)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp

REPS = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 20
WARMUP = 3
M, M_NEW = 128, 64
ctx = ab.Context(0)
lib = ctx._lib
keep = []  # device arrays of the current point


def device(a):
    d = ctx.to_device(np.ascontiguousarray(a))
    keep.append(d)
    return d


def features(x):
    f = capi.Features()
    f.n, f.dim, f.n_scale_columns, f.eq_id, f.scales, f.is_measurement = x.shape[0], 3, 0, None, None, 0
    f.coords, f.location = device(x).ptr, capi.DEVICE
    return f


def columns(vectors, rows):
    """the vectors as the columns of a rows x len(vectors) column-major matrix in HBM (zero below a shorter vector)"""
    a = np.zeros((len(vectors), rows))
    for j, v in enumerate(vectors):
        a[j, :len(v)] = v
    return device(a)


class Side:
    """B problems: training features and targets, test features, new observations, and the calls in groups (one group
    per size class; a single group for equal sizes)"""

    def __init__(self, sizes, kernels, seed):
        rng = np.random.default_rng(seed)
        self.B, self.sizes, self.kernels = len(sizes), sizes, kernels
        self.x = [rng.uniform(0., 10., (n, 3)) for n in sizes]
        self.y = [np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) for x in self.x]
        self.train = [features(x) for x in self.x]
        self.y_dev = [device(y) for y in self.y]
        self.test = [features(rng.uniform(0., 10., (M, 3))) for _ in sizes]
        self.new = [features(rng.uniform(0., 10., (M_NEW, 3))) for _ in sizes]
        self.y_new = [rng.standard_normal(M_NEW) for _ in sizes]
        self.y_new_dev = [device(y) for y in self.y_new]
        self.groups = abgp._size_classes(sizes)
        self.n_pad = [max(sizes[b] for b in g) for g in self.groups]
        self.Y = [columns([self.y[b] for b in g], n) for g, n in zip(self.groups, self.n_pad)]
        self.Y_new = [columns([self.y_new[b] for b in g], M_NEW) for g in self.groups]
        self.mean = device(np.zeros(M * self.B))
        self.second = device(np.zeros(M * M * self.B))

    def arr(self, items, g):
        return (C.c_void_p * len(g))(*[C.addressof(items[b]) if isinstance(items[b], capi.Features) else items[b] for b in g])

    def fit(self, entry):
        handles = [None] * self.B
        for g, n, Y in zip(self.groups, self.n_pad, self.Y):
            out, status = (C.c_void_p * len(g))(), (C.c_int * len(g))()
            rc = entry(ctx._h, len(g), self.arr(self.kernels, g), self.arr(self.train, g), C.c_void_p(Y.ptr), n, None, 0, out, None, 0, None, status)
            assert rc == capi.AGP_OK and not any(status)
            for j, b in enumerate(g):
                handles[b] = out[j]
        return handles

    def fit_loop(self):
        handles = []
        for b in range(self.B):
            h = C.c_void_p()
            rc = lib.agp_fit_create(ctx._h, self.kernels[b], C.byref(self.train[b]), C.c_void_p(self.y_dev[b].ptr), None, C.byref(h), None, None)
            assert rc == capi.AGP_OK
            handles.append(h.value)
        return handles

    def predict(self, handles, mode):
        per = M if mode == 1 else M * M
        first = 0
        for g in self.groups:  # (the outputs of a group lie behind those of the groups before it)
            status = (C.c_int * len(g))()
            rc = lib.agp_predict_batch(ctx._h, len(g), self.arr(self.kernels, g), self.arr(handles, g), self.arr(self.test, g), mode,
                                       C.c_void_p(self.mean.ptr + 8 * M * first), M, C.c_void_p(self.second.ptr + 8 * per * first), per,
                                       capi.DEVICE, status)
            assert rc == capi.AGP_OK and not any(status)
            first += len(g)

    def predict_loop(self, handles, mode):
        for b in range(self.B):
            mean, second = C.c_void_p(self.mean.ptr + 8 * M * b), C.c_void_p(self.second.ptr + 8 * M * M * b)
            if mode == 0:
                rc = lib.agp_predict_mean(ctx._h, self.kernels[b], handles[b], C.byref(self.test[b]), mean, capi.DEVICE)
            elif mode == 1:
                rc = lib.agp_predict_marginal(ctx._h, self.kernels[b], handles[b], C.byref(self.test[b]), mean, second, capi.DEVICE)
            else:
                rc = lib.agp_predict_joint(ctx._h, self.kernels[b], handles[b], C.byref(self.test[b]), mean, second, capi.DEVICE)
            assert rc == capi.AGP_OK

    def update(self, handles):
        grown = []
        for g, Y in zip(self.groups, self.Y_new):
            out, status = (C.c_void_p * len(g))(), (C.c_int * len(g))()
            rc = lib.agp_fit_update_batch(ctx._h, len(g), self.arr(self.kernels, g), self.arr(handles, g), self.arr(self.new, g), C.c_void_p(Y.ptr),
                                          M_NEW, None, 0, out, None, 0, None, status)
            assert rc == capi.AGP_OK and not any(status)
            grown.extend(out)
        return grown

    def update_loop(self, handles):
        grown = []
        for b in range(self.B):
            h = C.c_void_p()
            rc = lib.agp_fit_update(ctx._h, self.kernels[b], handles[b], C.byref(self.new[b]), C.c_void_p(self.y_new_dev[b].ptr), None, C.byref(h),
                                    None, None)
            assert rc == capi.AGP_OK
            grown.append(h.value)
        return grown


def destroy(handles):
    for h in handles:
        lib.agp_fit_destroy(C.c_void_p(h))


def times(fns):
    """REPS timings (ms) of each callable, alternating them so that all see the same machine"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(REPS):
        for fn, o in zip(fns, out):
            t = time.perf_counter()
            fn()
            ctx.synchronize()
            o.append((time.perf_counter() - t) * 1e3)
    return out


print(f"# median of {REPS} calls after {WARMUP} warm-up calls, ms; M = {M} test points, m = {M_NEW} new observations per problem")
print("# ragged = one batched call per size class; loop = B single calls on the same problems; equal = one batch of B fits of the largest size")
print("| sizes | B | classes | verb | ragged ms | loop ms (min .. max) | loop / ragged | equal ms | ragged / equal |")
print("|---|---|---|---|---|---|---|---|---|")
for lo, hi in ((129, 512), (400, 512)):
    for B in (8, 32, 256):
        sizes = [int(n) for n in np.random.default_rng(1000 * lo + B).integers(lo, hi + 1, B)]
        models = [ab.gp_from_covariance(ab.Matern52(1.5 + 0.5 * b / B, 1.0) + ab.IndependentNoise(0.1 + 0.05 * b / B), context=ctx) for b in range(B)]
        kernels = [ctx.private_kernel(mod.covariance_function_) for mod in models]
        ragged, equal = Side(sizes, kernels, B), Side([max(sizes)] * B, kernels, B + 1)
        rows = [("fit", lambda: destroy(ragged.fit(lib.agp_fit_create_batch_ragged)), lambda: destroy(ragged.fit_loop()),
                 lambda: destroy(equal.fit(lib.agp_fit_create_batch)))]
        hr, hl, he = ragged.fit(lib.agp_fit_create_batch_ragged), ragged.fit_loop(), equal.fit(lib.agp_fit_create_batch)
        for mode, name in enumerate(("predict mean", "predict marginal", "predict joint")):
            rows.append((name, lambda mode=mode: ragged.predict(hr, mode), lambda mode=mode: ragged.predict_loop(hl, mode),
                         lambda mode=mode: equal.predict(he, mode)))
        rows.append(("update", lambda: destroy(ragged.update(hr)), lambda: destroy(ragged.update_loop(hl)), lambda: destroy(equal.update(he))))
        for verb, f_ragged, f_loop, f_equal in rows:
            tr, tl, te = times([f_ragged, f_loop, f_equal])
            mr, ml, me = statistics.median(tr), statistics.median(tl), statistics.median(te)
            print(f"| {lo}..{hi} | {B} | {len(ragged.groups)} | {verb} | {mr:.3f} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {ml / mr:.1f} | {me:.3f} | "
                  f"{mr / me:.2f} |", flush=True)
        destroy(hr + hl + he)
        for k in kernels:
            lib.agp_kernel_destroy(k)
        del ragged, equal
        keep.clear()
ctx.close()
