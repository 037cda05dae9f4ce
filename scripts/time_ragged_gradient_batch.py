"""The exact likelihood gradients of B small problems of UNEQUAL sizes: the ragged batched entries (one
agp_nll_gradient_batch_ragged / agp_loo_nll_gradient_batch_ragged call per size class ceil(n_b / 128), as
ab.log_likelihood_gradient_batch / leave_one_out_likelihood_gradient_batch make them) against
  (a) the loop over agp_nll_gradient / agp_loo_nll_gradient on the same problems in the same process - the only route a
      caller with unequal sizes had before - and
  (b) ONE equal-size batch (agp_nll_gradient_batch / agp_loo_nll_gradient_batch) of B problems that all have the largest
      size of the draw: what the split into classes and the padding cost against a batch that needs neither.

Shapes: B in {8, 32, 256} problems with sizes drawn uniformly from 129..512 (three classes) and from 400..512 (one class),
seeded.  Covariance: 3-D Matern-5/2 + independent noise with a different parameter vector per problem (one tree: the
one-launch path of the covariance kernels), P = 3 slots.  Three verbs: the log-likelihood gradient, the leave-one-out
gradient, and the leave-one-out value-only path (no slots, no mean weights).  Every input lives in HBM
(agp_features.location = AGP_DEVICE: launches and device work, the table uploads and the result downloads of each call).
Per point: 3 warm-up calls, then the MEDIAN wall-clock time of REPS calls, the three sides alternating; the loop's spread
(min .. max of its REPS) is printed beside it as the run-to-run margin.
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


class Side:
    """B problems: features and targets in HBM, slot tables, and the calls in groups (one group per size class; a single
    group for equal sizes)"""

    def __init__(self, sizes, kernels, tables, n_slots, seed):
        rng = np.random.default_rng(seed)
        self.B, self.sizes, self.kernels, self.tables, self.P = len(sizes), sizes, kernels, tables, n_slots
        self.x = [rng.uniform(0., 10., (n, 3)) for n in sizes]
        self.y = [np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) for x in self.x]
        self.train = [features(x) for x in self.x]
        self.y_dev = [device(y) for y in self.y]
        self.groups = abgp._size_classes(sizes)
        self.n_pad = [max(sizes[b] for b in g) for g in self.groups]
        self.Y = []
        for g, n in zip(self.groups, self.n_pad):  # the targets of a group as the columns of an n x len(g) matrix
            a = np.zeros((len(g), n))
            for j, b in enumerate(g):
                a[j, :sizes[b]] = self.y[b]
            self.Y.append(device(a))
        self.value, self.grad, self.vec = np.zeros(self.B), np.zeros((self.B, n_slots)), np.zeros((self.B, max(sizes)))

    def arr(self, items, g):
        return (C.c_void_p * len(g))(*[C.addressof(items[b]) if isinstance(items[b], (capi.Features, C.Array)) else items[b] for b in g])

    def batch(self, entry, slots=True):
        for g, n, Y in zip(self.groups, self.n_pad, self.Y):
            k = len(g)
            status = (C.c_int * k)()
            n_slots = (C.c_int * k)(*([self.P if slots else 0] * k))
            rc = entry(ctx._h, k, self.arr(self.kernels, g), self.arr(self.train, g), C.c_void_p(Y.ptr), n, None, 0, n_slots,
                       self.arr(self.tables, g) if slots else None, None, 0, abgp._ptr(self.value), abgp._ptr(self.grad), self.P,
                       abgp._ptr(self.vec) if slots else None, self.vec.shape[1], status)
            assert rc == capi.AGP_OK and not any(status)

    def loop(self, entry, slots=True):
        v = C.c_double()
        for b in range(self.B):
            rc = entry(ctx._h, self.kernels[b], C.byref(self.train[b]), C.c_void_p(self.y_dev[b].ptr), None, self.P if slots else 0,
                       self.tables[b] if slots else None, None, 0, C.byref(v), abgp._ptr(self.grad[b]),
                       abgp._ptr(self.vec[b]) if slots else None)
            assert rc == capi.AGP_OK
            self.value[b] = v.value


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


print(f"# median of {REPS} calls after {WARMUP} warm-up calls, ms; P = 3 slots; inputs resident in HBM")
print("# ragged = one batched call per size class; loop = B single calls on the same problems; equal = one batch of B problems of the largest size")
print("| sizes | B | classes | verb | ragged ms | loop ms (min .. max) | loop / ragged | equal ms | ragged / equal |")
print("|---|---|---|---|---|---|---|---|---|")
for lo, hi in ((129, 512), (400, 512)):
    for B in (8, 32, 256):
        sizes = [int(n) for n in np.random.default_rng(1000 * lo + B).integers(lo, hi + 1, B)]
        models = [ab.gp_from_covariance(ab.Matern52(1.5 + 0.5 * b / B, 1.0) + ab.IndependentNoise(0.1 + 0.05 * b / B), context=ctx) for b in range(B)]
        kernels = [ctx.private_kernel(mod.covariance_function_) for mod in models]
        slot_lists = [mod.covariance_function_.param_slots()[0] for mod in models]
        P = len(slot_lists[0])
        assert P == 3
        tables = [(capi.GradientSlot * P)(*[capi.GradientSlot(node, p) for node, p, _ in s]) for s in slot_lists]
        ragged, equal = Side(sizes, kernels, tables, P, B), Side([max(sizes)] * B, kernels, tables, P, B + 1)
        rows = [
            ("log-likelihood gradient", lambda: ragged.batch(lib.agp_nll_gradient_batch_ragged), lambda: ragged.loop(lib.agp_nll_gradient),
             lambda: equal.batch(lib.agp_nll_gradient_batch)),
            ("leave-one-out gradient", lambda: ragged.batch(lib.agp_loo_nll_gradient_batch_ragged), lambda: ragged.loop(lib.agp_loo_nll_gradient),
             lambda: equal.batch(lib.agp_loo_nll_gradient_batch)),
            ("leave-one-out value only", lambda: ragged.batch(lib.agp_loo_nll_gradient_batch_ragged, False),
             lambda: ragged.loop(lib.agp_loo_nll_gradient, False), lambda: equal.batch(lib.agp_loo_nll_gradient_batch, False)),
        ]
        for verb, f_ragged, f_loop, f_equal in rows:
            tr, tl, te = times([f_ragged, f_loop, f_equal])
            mr, ml, me = statistics.median(tr), statistics.median(tl), statistics.median(te)
            print(f"| {lo}..{hi} | {B} | {len(ragged.groups)} | {verb} | {mr:.3f} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {ml / mr:.1f} | {me:.3f} | "
                  f"{mr / me:.2f} |", flush=True)
        for k in kernels:
            lib.agp_kernel_destroy(k)
        del ragged, equal
        keep.clear()
ctx.close()
