"""The leave-one-group-out likelihood and its exact gradient for B small problems: agp_logo_nll_gradient_batch (one call per
size class ceil(n_b / 128), as ab.leave_one_group_out_likelihood_gradient_batch makes them; the group blocks of all problems
of a call pooled into one chain per size class of groups) against the loop over agp_logo_nll_gradient_typed on the same
problems in the same process - the only route before the batched entry, and the reference for the ratio.

Cases: problems of N = 512 with groups of 16; problems of N = 512 with ragged groups of 1..64; sizes drawn from 129..512
(three classes) with groups of 16.  B in {8, 32, 256}; both predict types; value + gradient (P = 3 slots and the mean
weights) and the value alone.  Covariance: 3-D Matern-5/2 + independent noise with a parameter vector per problem.  Every
input lives in HBM (agp_features.location = AGP_DEVICE).  Per point: 3 warm-up calls, then the MEDIAN wall-clock time of
REPS calls, the two sides alternating; the loop's spread (min .. max) is printed beside it.  Then the stages of ONE profiled
batched call per case at B = 32 (agp_last_stage_ms, whole-batch times, summed over the size classes).
Arguments: REPS (default 10)."""
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

REPS = max(3, int(sys.argv[1])) if len(sys.argv) > 1 else 10
WARMUP = 3
P = 3
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


def grouping(n, rng, ragged):
    """(offsets, indices) of groups of 16 (the last one shorter) or of ragged sizes 1..64, over a random permutation"""
    perm = rng.permutation(n).astype(np.int64)
    sizes, at = [], 0
    while at < n:
        m = min(n - at, int(rng.integers(1, 65)) if ragged else 16)
        sizes.append(m)
        at += m
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), perm


class Side:
    def __init__(self, sizes, kernels, tables, ragged, seed):
        rng = np.random.default_rng(seed)
        self.B, self.sizes, self.kernels, self.tables = len(sizes), sizes, kernels, tables
        self.x = [rng.uniform(0., 10., (n, 3)) for n in sizes]
        self.y = [np.sin(x).sum(axis=1) + 0.1 * np.cos(10. * x[:, 0]) for x in self.x]
        self.train = [features(x) for x in self.x]
        self.y_dev = [device(y) for y in self.y]
        self.groups = [grouping(n, rng, ragged) for n in sizes]
        self.classes = abgp._size_classes(sizes)
        self.n_pad = [max(sizes[b] for b in g) for g in self.classes]
        self.Y = []
        for g, n in zip(self.classes, self.n_pad):  # the targets of a class as the columns of an n x len(g) matrix
            a = np.zeros((len(g), n))
            for j, b in enumerate(g):
                a[j, :sizes[b]] = self.y[b]
            self.Y.append(device(a))
        self.value, self.grad, self.vec = np.zeros(self.B), np.zeros((self.B, P)), np.zeros((self.B, max(sizes)))

    def arr(self, items, g):
        return (C.c_void_p * len(g))(*[C.addressof(items[b]) if isinstance(items[b], (capi.Features, C.Array)) else items[b] for b in g])

    def batch(self, ptype, slots=True):
        for g, n, Y in zip(self.classes, self.n_pad, self.Y):
            k = len(g)
            status = (C.c_int * k)()
            n_slots = (C.c_int * k)(*([P if slots else 0] * k))
            n_groups = (C.c_int64 * k)(*[len(self.groups[b][0]) - 1 for b in g])
            offsets = (C.c_void_p * k)(*[self.groups[b][0].ctypes.data for b in g])
            indices = (C.c_void_p * k)(*[self.groups[b][1].ctypes.data for b in g])
            rc = lib.agp_logo_nll_gradient_batch(ctx._h, k, self.arr(self.kernels, g), self.arr(self.train, g), C.c_void_p(Y.ptr), n, None, 0,
                                                 n_groups, offsets, indices, ptype, n_slots, self.arr(self.tables, g) if slots else None, None,
                                                 0, abgp._ptr(self.value), abgp._ptr(self.grad), P, abgp._ptr(self.vec) if slots else None,
                                                 self.vec.shape[1], None, status)
            assert rc == capi.AGP_OK and not any(status), (rc, list(status))

    def loop(self, ptype, slots=True):
        v = C.c_double()
        for b in range(self.B):
            off, ind = self.groups[b]
            rc = lib.agp_logo_nll_gradient_typed(ctx._h, self.kernels[b], C.byref(self.train[b]), C.c_void_p(self.y_dev[b].ptr), None,
                                                 len(off) - 1, abgp._ptr(off), abgp._ptr(ind), ptype, P if slots else 0,
                                                 self.tables[b] if slots else None, None, 0, C.byref(v), abgp._ptr(self.grad[b]),
                                                 abgp._ptr(self.vec[b]) if slots else None, None)
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


def stage_ms(k):
    v = C.c_double()
    lib.agp_last_stage_ms(ctx._h, k, C.byref(v))
    return v.value


CASES = [("N = 512, groups of 16", lambda B, rng: [512] * B, False),
         ("N = 512, ragged groups 1..64", lambda B, rng: [512] * B, True),
         ("N in 129..512, groups of 16", lambda B, rng: [int(n) for n in rng.integers(129, 513, B)], False)]
TYPES = [("joint", capi.PREDICT_JOINT), ("marginal", capi.PREDICT_MARGINAL)]
STAGES = [(0, "gram"), (1, "factor"), (2, "alpha, R"), (6, "R^T R"), (8, "blocks, sums, u, H"), (9, "H C^T"), (7, "contraction")]

print(f"# median of {REPS} calls after {WARMUP} warm-up calls, ms; P = 3 slots; inputs resident in HBM")
print("# batch = one agp_logo_nll_gradient_batch call per size class; loop = B agp_logo_nll_gradient_typed calls on the same problems")
print("| case | B | classes | type | verb | batch ms | loop ms (min .. max) | loop / batch |")
print("|---|---|---|---|---|---|---|---|")
profiles = []
for label, draw, ragged in CASES:
    for B in (8, 32, 256):
        sizes = draw(B, np.random.default_rng(1000 + B))
        models = [ab.gp_from_covariance(ab.Matern52(1.5 + 0.5 * b / B, 1.0) + ab.IndependentNoise(0.1 + 0.05 * b / B), context=ctx) for b in range(B)]
        kernels = [ctx.private_kernel(mod.covariance_function_) for mod in models]
        slot_lists = [mod.covariance_function_.param_slots()[0] for mod in models]
        assert len(slot_lists[0]) == P
        tables = [(capi.GradientSlot * P)(*[capi.GradientSlot(node, p) for node, p, _ in s]) for s in slot_lists]
        side = Side(sizes, kernels, tables, ragged, B)
        for tname, ptype in TYPES:
            for verb, slots in (("value + gradient", True), ("value only", False)):
                tb, tl = times([lambda: side.batch(ptype, slots), lambda: side.loop(ptype, slots)])
                mb, ml = statistics.median(tb), statistics.median(tl)
                print(f"| {label} | {B} | {len(side.classes)} | {tname} | {verb} | {mb:.3f} | {ml:.3f} ({min(tl):.3f} .. {max(tl):.3f}) | {ml / mb:.1f} |",
                      flush=True)
        if B == 32:  # one profiled call per case and type: whole-batch stage times, summed over the size classes
            lib.agp_set_profiling(ctx._h, 1)
            for tname, ptype in TYPES:
                total = {k: 0. for k, _ in STAGES}
                for g in side.classes:
                    one = Side.__new__(Side)
                    one.__dict__.update(side.__dict__)
                    j = side.classes.index(g)
                    one.classes, one.n_pad, one.Y = [g], [side.n_pad[j]], [side.Y[j]]
                    one.batch(ptype, True)
                    for k, _ in STAGES:
                        total[k] += stage_ms(k)
                profiles.append((label, tname, total))
            lib.agp_set_profiling(ctx._h, 0)
        for k in kernels:
            lib.agp_kernel_destroy(k)
        del side
        keep.clear()
print()
print("# one profiled value + gradient call at B = 32, ms per stage (whole batch)")
print("| case | type | " + " | ".join(name for _, name in STAGES) + " |")
print("|---|---|" + "---|" * len(STAGES))
for label, tname, total in profiles:
    print(f"| {label} | {tname} | " + " | ".join(f"{total[k]:.3f}" for k, _ in STAGES) + " |")
ctx.close()
