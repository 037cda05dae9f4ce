"""Shared by tests/test_contraction_bounds_host.py and tests/test_contraction_kernels_gpu.py: the reference, the bound, the
cases and the ctypes prototypes for the gradient contraction kernels - contract_tile (csrc/contract.h) driven by
eval_pair_tangent (csrc/cov_eval.h) - run on the caller's weights through agp_debug_contract_dense, _batched and _sparse
(csrc/debug_api.hip), which call the launchers of csrc/contract_internal.h that the gradient entries call.  Nothing here is
measured on a GPU.

Reference.  eval_tangent() restates eval_pair_tangent in numpy, for all pairs of two feature sets at once: the metric
distances and the equality predicate in fp64 in the kernel's operation order (they are INPUTS of the leaf formulas; the
angular distance is the longdouble arccos of the fp64 cosine), then every leaf value, every analytic parameter derivative
and the composites (sum; product with the `lhs == 0` short circuit and the `defined` bits; MeasurementOnly; TypePair) in
np.longdouble.  The same function runs in fp64 (T = np.float64) for the host file's restatement in kernel order.  The
three weights are restated the same way: C_ij - a_i a_j, S_ij - (u_i a_j + a_i u_j) / 2 and W_ij, and sum mult w dk is
taken in np.longdouble (mult: 2 below the diagonal of a lower contraction, 1 on it, 1 everywhere in a rectangular one).

Scale.  Per slot sum mult |w|* |dk|*: |w|* the sum of the absolute values of the weight's terms (|C_ij| + |a_i a_j|), |dk|*
from the same recursion with absolute values at every sum and at both halves of every product rule.  It cannot cancel.

Bound.  |got - ref| <= (d_sum + c_eval) 2^-53 scale.  U = 2^-53 is one rounding.

  d_sum, the roundings one term can pass through between the pair and the result (Higham, Accuracy and Stability of
  Numerical Algorithms, section 3.1: a sum in which no term passes through more than k roundings is within about k U sum |terms|
  of the exact one, whatever the order):
      3   the weight: a_i a_j and the subtraction (2), or u_i a_j, a_i u_j, their sum and the subtraction - the halving and
          the doubling of an off-diagonal pair are exact (at most 3, relative to |w|*)
      1   the product w dk (none when it is fused into the addition)
     16   a lane adds its CT / 4 = 16 columns of the tile one after the other
      6   butterfly steps over the 64 lanes of a wave (reduce_tile)
      3   additions across the four waves
      ceil(tiles / 256)   serial additions of a thread of reduce_partials, then
      8   tree steps over its 256 threads
      1   the final scale (a power of two in every caller, counted all the same)
      3   sparse_grad_reduce_kernel only: the three-term combination (factors -1/2, -1, -1/2 exact, three additions)
  d_sum(tiles) = 38 + ceil(tiles / 256), + 3 for the combination.

  c_eval, the relative error of a computed dk against the longdouble value from the same fp64 distances, in units of U and
  relative to |dk|*.  An error of 1 ulp is 2 U.  Per leaf, with e_q the relative error of q = dist / l:
      e_dist  Euclidean, dim > 1: (dim + 1): the kernel may fuse t * t into the running sum and the restatement does not -
              either value is within dim U of the exact sum of squares of the same differences t, the square root halves
              that and adds its own rounding on each side ((2 dim) / 2 + 1); dim = 1: |x - y| is the same operation, 0.
              Radial: 0 (integer norms, below).  Angular: 3 (acos_fast: 1.1 ulp = 2.2 U; the cosine is one division
              of exact integers on both sides).
      e_q     e_dist + 1 (the division), + 2 for Matern (the constant sqrt(3) or sqrt(5) and its product)
      exp_neg 1.5 ulp = 3 U, and an argument error e_t in t = q^2 or q amplified by t: exp(-t (1 + e)) = exp(-t) (1 - t e)
      SQUARED_EXPONENTIAL  t = q^2, e_t = 2 e_q + 1;  dshape_dl = e 2 q q / l and sigma sigma (.) : 2 e_q + 5 more
      EXPONENTIAL          t = q,   e_t = e_q;        e q / l, sigma sigma (.)                  : e_q + 4
      MATERN32             t = q,   e_t = e_q;        q q e / l, (1 + q) e, sigma sigma (.)     : 2 e_q + 5
      MATERN52             t = q,   e_t = e_q;        q q (1 + q) (1/3) e / l, sigma sigma (.)  : 3 e_q + 8
      c_leaf = 3 + T e_t + (the operations), T the largest exponent argument of the case, computed from its own pairs and
      rounded up to an integer (Case.t_cap: 1 .. 7 over the cases here; check_inputs asserts the reference's largest
      argument against it, and it against T_CAP = 32)
      CONSTANT, INDEPENDENT_NOISE, NUGGET: 2 p is exact - 1.  POLYNOMIAL of order o: 2 s xp yp with xp, yp after o - 1
      products each - 2 o + 2.  SCALING: tx fy + fx ty, relative to |tx fy| + |fx ty| - 3.
  Composites, to first order and relative to the starred magnitudes: a sum is as good as its worse side plus its own
  rounding, a product rule tl r + l tr carries the errors of both factors plus three roundings.  Both are covered by
      c_eval = sum over the leaves of c_leaf + 2 (number of composite nodes) + 1,
  the 1 for the longdouble reference (2^-11 U per operation) and the conversion of the compared value.

Conditions on the inputs, all asserted by check_inputs() without a GPU:
  * Radial and angular cases use integer coordinates whose norms are integers: signed permutations of (1,2,2), (2,3,6),
    (1,4,8), (4,4,7), (2,6,9), (6,6,7) scaled by 1/2, 1 or 2.  |x|^2 and every partial sum of it are exact, so the norm is
    exact with or without fused multiply-adds, | |x| - |y| | is exact, every dot product is exact, and every cosine is
    one division of exact numbers: exactly +-1 (parallel points, the diagonal included: the c > 1 - eps and c < -1 + eps
    branches on purpose) or within [-0.99, 0.99].  No case depends on which side of 1 - 1e-16 a rounded cosine lands.
  * Euclidean cases use random coordinates with planted duplicates (gram_path_cases.planted_symmetric, planted_ids).
  * The largest exponent argument of every case is at most its t_cap, and that at most T_CAP = 32.  The one exception is
    marked (Case.far): a point
    1e200 away, whose squared distance overflows, under noise * squared_exponential - there the left factor is exactly 0,
    the kernel must not look at the right one (0 * inf), the reference's dk is exactly 0 for every slot on those pairs
    (asserted), so they carry no error and t_cap speaks of the other pairs.
  * Noise and nugget cases plant duplicates, with ids on both views, on one view only (the comparison falls back to the
    coordinates) and without ids.

Canaries (the GPU file): the strict upper triangle of a lower weight, its padding rows (ld > n), the tangent buffer beyond n
and beyond the columns in use, and u without LOO are NaN; out beyond n_slots and the partials beyond the tiles keep their
bits; the partials of a phantom tile of a ragged batch are exactly 0.
"""
import ctypes as C
import functools
import math

import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
import gram_path_cases as gp
from gram_path_cases import HAVE_LONGDOUBLE, Elevation, features, noise, planted_ids, radial  # noqa: F401

U = 2.0 ** -53
LD = np.longdouble
GRAD_GROUP, CT = 4, 64  # csrc/contract.h
E, R, A = ab.EuclideanDistance, ab.RadialDistance, ab.AngularDistance
SE, EXP, M32, M52 = capi.OP_SQUARED_EXPONENTIAL, capi.OP_EXPONENTIAL, capi.OP_MATERN32, capi.OP_MATERN52
T_CAP = 32.


def lower_tiles(n):
    t = -(-n // CT)
    return t * (t + 1) // 2


# ---- the bound -------------------------------------------------------------------------------------------------------
def d_sum(tiles, combination=False):
    return 3 + 1 + 16 + 6 + 3 + -(-tiles // 256) + 8 + 1 + (3 if combination else 0)


def c_leaf(nd, dim, t_cap):
    op = nd["op"]
    if op <= M52:
        e_dist = {capi.METRIC_EUCLIDEAN: (dim + 1 if dim > 1 else 0), capi.METRIC_RADIAL: 0, capi.METRIC_ANGULAR: 3}[nd["metric"]]
        e_q = e_dist + 1 + (0 if op in (SE, EXP) else 2)
        e_t, ops = {SE: (2 * e_q + 1, 2 * e_q + 5), EXP: (e_q, e_q + 4), M32: (e_q, 2 * e_q + 5), M52: (e_q, 3 * e_q + 8)}[op]
        return 3 + t_cap * e_t + ops
    if op == capi.OP_POLYNOMIAL:
        return 2 * nd["order"] + 2
    if op == capi.OP_SCALING:
        return 3
    return 1


def c_eval(nodes, dim, t_cap):
    leaves = sum(c_leaf(nd, dim, t_cap) for nd in nodes if nd["op"] <= capi.OP_SCALING)
    return leaves + 2 * sum(1 for nd in nodes if nd["op"] > capi.OP_SCALING) + 1


# ---- the reference ---------------------------------------------------------------------------------------------------
def plain_nodes(cov):
    return [dict(op=nd.op, metric=nd.metric, column=nd.column, order=nd.order, params=[float(p) for p in nd.params])
            for nd in cov.program_nodes()]


def distances(fr, fc, metrics):
    """{metric: rows x cols distances}: fp64 in the operation order of eval_pair_tangent; the angular one is the longdouble
    arccos of the fp64 cosine.  Coordinates beyond dim are the zeros of the padded Point: they change no bit."""
    x, y = fr.coords, fc.coords
    dim = x.shape[1]
    out = {}
    with np.errstate(all="ignore"):
        if capi.METRIC_EUCLIDEAN in metrics:
            if dim == 1:
                out[capi.METRIC_EUCLIDEAN] = np.abs(x[:, None, 0] - y[None, :, 0])
            else:
                s = np.zeros((fr.n, fc.n))
                for d in range(dim):
                    t = x[:, None, d] - y[None, :, d]
                    s = s + t * t
                out[capi.METRIC_EUCLIDEAN] = np.sqrt(s)
        if capi.METRIC_RADIAL in metrics or capi.METRIC_ANGULAR in metrics:
            nx, ny = np.zeros(fr.n), np.zeros(fc.n)
            for d in range(dim):
                nx = nx + x[:, d] * x[:, d]
                ny = ny + y[:, d] * y[:, d]
            nx, ny = np.sqrt(nx), np.sqrt(ny)
            out[capi.METRIC_RADIAL] = np.abs(nx[:, None] - ny[None, :])
        if capi.METRIC_ANGULAR in metrics:
            dot = np.zeros((fr.n, fc.n))
            for d in range(dim):
                dot = dot + x[:, None, d] * y[None, :, d]
            c = dot / (nx[:, None] * ny[None, :])
            eps = 1e-16
            out["cos"] = c
            out[capi.METRIC_ANGULAR] = np.where(c > 1. - eps, LD(0), np.where(c < -1. + eps, LD(math.pi), np.arccos(c.astype(LD))))
    return out


def equality(fr, fc):
    if fr.eq_id is not None and fc.eq_id is not None:
        return fr.eq_id[:, None] == fc.eq_id[None, :]
    return np.all(fr.coords[:, None, :] == fc.coords[None, :, :], axis=2)


def eval_tangent(nodes, slots, fr, fc, tr=None, tc=None, T=LD, mut=()):
    """dk / dslot for every pair (row of fr, column of fc): (dk, dk_abs, value, t) - lists of rows x cols arrays per slot,
    the value, and the largest exponent argument of the pair over the radial leaves (fp64).  tr / tc: rows x columns and
    cols x columns tangent matrices of the AGP_OP_SCALING slots.  T: np.longdouble (the reference) or np.float64.
    mut: the faults of tests/test_contraction_bounds_host.py that live in the evaluation."""
    n, m, G = fr.n, fc.n, len(slots)
    D = distances(fr, fc, {nd["metric"] for nd in nodes if nd["op"] <= M52})
    equal = equality(fr, fc) if any(nd["op"] in (capi.OP_INDEPENDENT_NOISE, capi.OP_NUGGET) for nd in nodes) else None
    both_meas = bool(fr.is_measurement) and bool(fc.is_measurement)
    zero, yes = np.zeros((n, m), dtype=T), np.ones((n, m), dtype=bool)
    tmax = np.zeros((n, m))
    st = []  # entries [v, va, t (G), ta (G), defined]
    with np.errstate(all="ignore"):
        for t, nd in enumerate(nodes):
            op, p = nd["op"], nd["params"]
            if op <= capi.OP_SCALING:
                v, dp, fx, fy = zero, [zero] * 4, None, None
                if op <= M52:
                    dist, l, sigma = D[nd["metric"]].astype(T), T(p[0]), T(p[1])
                    if p[0] > 0.:
                        if op == SE:
                            q = dist / l
                            tt = q * q
                            e = np.exp(-tt)
                            shape, dshape = e, e * T(2.) * q * q / l
                        elif op == EXP:
                            q = np.abs(dist / l)
                            tt = q
                            e = np.exp(-q)
                            shape, dshape = e, e * q / l
                        elif op == M32:
                            q = T(np.sqrt(3.)) * dist / l
                            tt = q
                            e = np.exp(-q)
                            shape, dshape = (1 + q) * e, q * q * e / l
                        else:
                            q = T(np.sqrt(5.)) * dist / l
                            tt = q
                            e = np.exp(-q)
                            third = T(0.333) if "m52_third" in mut else T(1. / 3.)
                            shape, dshape = (1 + q + q * q * T(1. / 3.)) * e, q * q * (1 + q) * third * e / l
                        v = sigma * sigma * shape
                        dp = [sigma * sigma * dshape, T(2.) * sigma * shape, zero, zero]
                        tmax = np.fmax(tmax, tt.astype(np.float64))
                elif op == capi.OP_CONSTANT:
                    v, dp = zero + T(p[0]) * T(p[0]), [zero + T(2.) * T(p[0]), zero, zero, zero]
                elif op in (capi.OP_INDEPENDENT_NOISE, capi.OP_NUGGET):
                    v = np.where(equal, T(p[0]) * T(p[0]), T(0))
                    dp = [np.where(equal, T(2.) * T(p[0]), T(0)), zero, zero, zero]
                elif op == capi.OP_POLYNOMIAL:
                    xp, yp = np.ones((n, 1), dtype=T), np.ones((1, m), dtype=T)
                    x0, y0 = fr.coords[:, 0].astype(T)[:, None], fc.coords[:, 0].astype(T)[None, :]
                    dp = [zero] * 4
                    for q in range(nd["order"] + 1):
                        s = T(p[q])
                        v = v + s * s * xp * yp
                        dp[q] = T(2.) * s * xp * yp
                        xp, yp = xp * x0, yp * y0
                else:
                    fx = fr.scales[:, nd["column"]].astype(T)[:, None]
                    fy = fc.scales[:, nd["column"]].astype(T)[None, :]
                    v = fx * fy + zero
                tg, ta = [], []
                for g, (node, param) in enumerate(slots):
                    if node != t:
                        tg.append(zero); ta.append(zero)
                    elif op == capi.OP_SCALING:
                        col = (param + 1) % tr.shape[1] if "next_tangent" in mut else param
                        a, b = tr[:, col].astype(T)[:, None] * fy, fx * tc[:, col].astype(T)[None, :]
                        tg.append(a + b); ta.append(np.abs(a) + np.abs(b))
                    else:
                        tg.append(dp[param]); ta.append(np.abs(dp[param]))
                st.append([v, np.abs(v), tg, ta, yes])
            elif op == capi.OP_SUM:
                r, l = st.pop(), st.pop()
                st.append([l[0] + r[0], l[1] + r[1], [a + b for a, b in zip(l[2], r[2])], [a + b for a, b in zip(l[3], r[3])],
                           l[4] | r[4]])
            elif op == capi.OP_PRODUCT:
                r, l = st.pop(), st.pop()
                both, live = l[4] & r[4], l[0] != 0

                def pick(b_live, b_zero, left, right):
                    return np.where(both, np.where(live, b_live, b_zero), np.where(l[4], left, np.where(r[4], right, T(0))))
                v = pick(l[0] * r[0], l[0], l[0], r[0])
                va = pick(l[1] * r[1], l[1], l[1], r[1])
                tg, ta = [], []
                for g in range(G):
                    tl, tr_, tla, tra = l[2][g], r[2][g], l[3][g], r[3][g]
                    rule = tl * r[0] + l[0] * tr_
                    zb = rule if "zero_branch" in mut else np.where(tl != 0, tl * r[0], T(0))
                    tg.append(pick(rule, zb, tl, tr_))
                    ta.append(pick(tla * r[1] + l[1] * tra, np.where(tl != 0, tla * r[1], T(0)), tla, tra))
                st.append([v, va, tg, ta, l[4] | r[4]])
            elif op == capi.OP_MEASUREMENT_ONLY:
                if not both_meas:
                    top = st[-1]
                    top[0], top[1] = zero, zero
                    if "meas_tangent" not in mut:
                        top[2], top[3] = [zero] * G, [zero] * G
            else:  # AGP_OP_TYPE_PAIR
                ax, ay = fr.scales[:, nd["column"]][:, None], fc.scales[:, nd["column"]][None, :]
                a, b = p[0], p[1]
                ok = ((ax == a) & (ay == b)) | ((ax == b) & (ay == a))
                top = st[-1]
                top[0], top[1] = np.where(ok, top[0], T(0)), np.where(ok, top[1], T(0))
                top[2] = [np.where(ok, a_, T(0)) for a_ in top[2]]
                top[3] = [np.where(ok, a_, T(0)) for a_ in top[3]]
                top[4] = top[4] & ok
    assert len(st) == 1
    return st[0][2], st[0][3], st[0][0], tmax


# ---- weights ------------------------------------------------------------------------------------------------------------
class Block:
    """One weight matrix of a contraction: rows rbase .. rbase + nr of the row features against columns cbase .. cbase + nc
    of the column features; M the nr x nc fp64 matrix part (a view into the case's buffer), a / u the vectors of the dense
    weights at those points, kind 'nll' / 'loo' / 'mat'."""

    def __init__(self, kind, rbase, cbase, M, lower, a=None, u=None):
        self.kind, self.rbase, self.cbase, self.M, self.lower, self.a, self.u = kind, rbase, cbase, M, lower, a, u
        self.nr, self.nc = M.shape

    def mult(self):
        if not self.lower:
            return np.ones((self.nr, self.nc))
        i, j = np.arange(self.nr)[:, None], np.arange(self.nc)[None, :]
        return np.where(i > j, 2., np.where(i == j, 1., 0.))

    def weight(self, T):
        """(w, |w|*), the unused upper triangle of a lower weight (NaN in the buffer) as 0"""
        keep = self.mult() > 0
        M = np.where(keep, self.M, 0.).astype(T)
        if self.kind == "mat":
            return M, np.abs(M)
        ai, aj = self.a.astype(T)[:, None], self.a.astype(T)[None, :]
        if self.kind == "nll":
            return np.where(keep, M - ai * aj, T(0)), np.where(keep, np.abs(M) + np.abs(ai * aj), T(0))
        ui, uj = self.u.astype(T)[:, None], self.u.astype(T)[None, :]
        w = M - T(0.5) * (ui * aj + ai * uj)
        wa = np.abs(M) + T(0.5) * (np.abs(ui * aj) + np.abs(ai * uj))
        return np.where(keep, w, T(0)), np.where(keep, wa, T(0))

    def tiles(self, row_major=False):
        """(bi, bj) in the order of the tile ids"""
        tr, tc = -(-self.nr // CT), -(-self.nc // CT)
        if self.lower:
            return [(bi, bj) for bi in range(tr) for bj in range(bi + 1)]
        if row_major:  # the fault: id decoded as bi = id / tiles_r, bj = id % tiles_r
            return [(i // tr, i % tr) for i in range(tr * tc)]
        return [(i % tr, i // tr) for i in range(tr * tc)]


def padded_matrix(M, ld, lower=False):
    """rows x cols M column-major at leading dimension ld >= rows in a flat buffer; padding rows - and the strict upper
    triangle when `lower` - NaN: (flat, the rows x cols view)"""
    rows, cols = M.shape
    assert ld >= rows
    flat = np.full(ld * cols, np.nan)
    view = flat.reshape((ld, cols), order="F")[:rows]
    view[:] = M
    if lower:
        view[np.triu_indices(rows, 1, cols)] = np.nan
    return flat, view


def padded_tangents(Tm, ld):
    """n x ntc tangent columns at ld > n with one more column, everything else NaN; None without columns"""
    if Tm is None:
        return None
    n, ntc = Tm.shape
    flat = np.full(ld * (ntc + 1), np.nan)
    flat.reshape((ld, ntc + 1), order="F")[:n, :ntc] = Tm
    return flat


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case:
    """One contraction: family 'dense_nll' / 'dense_loo' / 'sparse_sym' / 'sparse_rect' / 'sparse_groups'; cov, nodes, slots
    [(node, param)]; fr / fc the row / column FeatureSets (fc is fr in the symmetric families); tr / tc the tangent matrices
    (or None); blocks; the flat buffers the entry points take; t_cap."""
    far = False

    @property
    def t_cap(self):
        """what c_eval assumes for the largest exponent argument: the case's own, rounded up to an integer (at least 1)"""
        if getattr(self, "_t_cap", None) is None:
            self._t_cap = float(max(1, math.ceil(largest_exponent(self))))
        return self._t_cap

    @property
    def lower(self):
        return self.family != "sparse_rect"

    @property
    def tiles(self):
        return sum(len(b.tiles()) for b in self.blocks)

    @property
    def dim(self):
        return self.fr.dim

    def gamma(self, combination=False):
        return (d_sum(self.tiles, combination) + c_eval(self.nodes, self.dim, self.t_cap)) * U


def largest_exponent(case):
    """the largest exponent argument t (q^2 of a squared exponential, q of the others) over the radial leaves and the pairs
    the contraction visits, from the fp64 distances; pairs beyond T_CAP are the far pairs of a Case.far case (check_inputs)"""
    worst = 0.
    for b in case.blocks:
        fr, fc = _sub(case.fr, b.rbase, b.rbase + b.nr), _sub(case.fc, b.cbase, b.cbase + b.nc)
        D = distances(fr, fc, {nd["metric"] for nd in case.nodes if nd["op"] <= M52})
        live = b.mult() > 0
        for nd in case.nodes:
            if nd["op"] > M52 or nd["params"][0] <= 0.:
                continue
            with np.errstate(all="ignore"):
                q = np.asarray(D[nd["metric"]], dtype=np.float64) / nd["params"][0]
                t = q * q if nd["op"] == SE else np.abs(q) * {EXP: 1., M32: np.sqrt(3.), M52: np.sqrt(5.)}.get(nd["op"], 1.)
            ok = live & (t <= T_CAP)
            worst = max(worst, float(np.max(t[ok], initial=0.)))
    return worst


def rng_of(*key):
    return np.random.default_rng([_stable(k) if isinstance(k, str) else abs(int(k)) for k in key])


def _stable(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


TRIPLES = [(1, 2, 2), (2, 3, 6), (1, 4, 8), (4, 4, 7), (2, 6, 9), (6, 6, 7)]
INT_SCALES = [0.5, 1., 2.]


@functools.lru_cache(maxsize=1)
def integer_directions():
    """signed permutations of TRIPLES, thinned greedily so that two directions are antiparallel or at most 0.99 in cosine"""
    import itertools
    cand = []
    for t in TRIPLES:
        for perm in sorted(set(itertools.permutations(t))):
            for sg in itertools.product((1, -1), repeat=3):
                cand.append(tuple(float(s * c) for s, c in zip(sg, perm)))
    cand = sorted(set(cand), key=lambda v: (_stable(repr(v)), v))
    kept = []
    for v in cand:
        a = np.array(v)
        ok = True
        for w in kept:
            b = np.array(w)
            c = float(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
            if abs(c) > 0.99 and not np.array_equal(a * np.linalg.norm(b), -b * np.linalg.norm(a)):
                ok = False
                break
        if ok:
            kept.append(v)
    return np.array(kept)


def integer_points(n, seed):
    """n points direction * scale: every direction at every scale before any repeats (parallel pairs, cosine exactly 1), the
    antipodes among the directions (cosine exactly -1)"""
    dirs = integer_directions()
    rng = rng_of("int", seed)
    order = rng.permutation(len(dirs) * len(INT_SCALES))
    idx = np.resize(order, n)
    S = len(INT_SCALES)
    if n > 4:  # point 3 parallel to point 1 at another scale, point 4 antiparallel to it
        idx[3] = idx[1] // S * S + (idx[1] % S + 1) % S
        anti = np.flatnonzero(np.all(dirs == -dirs[idx[1] // S], axis=1))
        assert anti.size == 1
        idx[4] = anti[0] * S + idx[1] % S
    if n > 8:  # duplicates of points 0 and 2 (noise off the diagonal)
        idx[n - 1], idx[6] = idx[0], idx[2]
    return dirs[idx // len(INT_SCALES)] * np.array(INT_SCALES)[idx % len(INT_SCALES)][:, None]


def radial_any(op, length_scale, sigma, metric):
    """radial() for every (leaf, metric) the program format allows: the Python class refuses SquaredExponential over the
    angular metric (not positive definite), the kernel evaluates it like any other"""
    cov = gp.RADIALS[op](length_scale, sigma, None)
    cov.distance_metric_ = metric()
    return cov


def _scaling_tree():
    return ab.ScalingTerm(Elevation()) * ab.Constant(0.8) + radial(2, 6.0, 1.1, E) + noise()


def _variant_tree():
    """TYPE_PAIR gates: a term per pair of alternatives, and a product whose left operand the gate leaves undefined for
    every pair but (0, 1) - the product is then its right operand alone"""
    return (ab.only_for_alternatives(radial(0, 6.0, 1.2, E), 0, 0)
            + ab.only_for_alternatives(radial(1, 5.0, 0.9, E), 0, 1) * radial(2, 7.0, 1.1, E)
            + ab.only_for_alternatives(noise(), 1, 1))


# name: (builder, coordinates: 'e' random with planted duplicates / 'i' integer norms (dim 3) / 'p' dim 1 / 'v' variant /
# 'f' dim 2 with a far point, dims)
TREES = {}
for _op, _nm in enumerate(gp.RADIAL_IDS):
    TREES[f"{_nm}_e+noise"] = (lambda o=_op: radial(o, 6.0, 1.3, E) + noise(), "e")
    TREES[f"{_nm}_r+noise"] = (lambda o=_op: radial_any(o, 16.0, 1.2, R) + noise(), "i")
    TREES[f"{_nm}_a+noise"] = (lambda o=_op: radial_any(o, 1.7, 0.9, A) + noise(), "i")
TREES.update({
    "const+noise": (lambda: ab.Constant(0.7) + noise(), "e"),
    "m32_e+nugget": (lambda: radial(2, 6.0, 1.1, E) + ab.Nugget(0.2), "e"),
    "poly0+noise": (lambda: ab.Polynomial(0, 0.9) + noise(), "p"),
    "poly1+noise": (lambda: ab.Polynomial(1, 0.6) + noise(), "p"),
    "poly2+noise": (lambda: ab.Polynomial(2, 0.4) + noise(), "p"),
    "poly3+noise": (lambda: ab.Polynomial(3, 0.3) + noise(), "p"),
    "scaling": (_scaling_tree, "e"),
    "m32_r*m32_a": (lambda: radial_any(2, 16.0, 1.1, R) * radial_any(2, 1.9, 0.9, A) + noise(), "i"),
    "m52_e*m52_e": (lambda: radial(3, 6.0, 1.1, E) * radial(3, 9.0, 0.8, E), "e"),
    "radial*noise": (lambda: radial(3, 6.0, 1.1, E) * noise() + radial(1, 7.0, 0.6, E), "e"),
    "noise*radial": (lambda: noise() * radial(3, 6.0, 1.1, E) + radial(1, 7.0, 0.6, E), "e"),
    "m52_e+meas(noise)": (lambda: radial(3, 6.0, 1.0, E) + ab.measurement_only(noise()), "e"),
    "variant": (_variant_tree, "v"),
    "ten_slots": (lambda: ab.Constant(0.7) + radial(0, 6.0, 1.1, E) + radial(1, 7.0, 0.9, E) + radial(2, 8.0, 1.2, E)
                  + radial(3, 5.0, 0.8, E) + noise(), "e"),
    "nine_slots": (lambda: radial(0, 6.0, 1.1, E) + radial(1, 7.0, 0.9, E) + radial(2, 8.0, 1.2, E) + radial(3, 5.0, 0.8, E)
                   + noise(), "e"),
    "m32_e+noise3": (lambda: radial(2, 6.0, 1.3, E) + noise(), "e"),
    "far:noise*se": (lambda: noise() * radial(0, 6.0, 1.1, E) + ab.Nugget(0.2), "f"),
})
TREE_NAMES = list(TREES)
ID_MODES = [None, "both", "rows", "cols"]


def elevation_tangents(cov, coords):
    """the tangent columns of the tree's ScalingTerm(Elevation) slots, analytic: d f / d center = factor [center > c],
    d f / d factor = max(center - c, 0)"""
    _, columns = cov.param_slots()
    if not columns:
        return None
    c0 = np.asarray(coords, dtype=np.float64)[:, 0]
    cols = []
    for fn, name in columns:
        center, factor = fn.get_params()["center"], fn.get_params()["factor"]
        cols.append(factor * (center > c0) if name == "center" else np.maximum(center - c0, 0.))
    return np.column_stack(cols).astype(np.float64)


def make_features(name, n, dim, seed, meas, ids=False, other=None):
    """(cov, FeatureSet, coordinates) of `n` points for tree `name`.  ids: explicit equality ids - all distinct but the last
    point's, which is point 0's, and point 6's, which is point 2's (noise between different coordinates); planted coordinate duplicates keep different ids."""
    build, kind = TREES[name]
    cov = build()
    if kind == "i":
        x = integer_points(n, seed)
    elif kind == "v":
        rng = rng_of("var", seed, n)
        x = rng.uniform(0.5, 10., (n, 3))
        alt = rng.integers(0, 2, n)
        if n > 4:
            x[3], alt[3] = x[1], alt[1]
        fs = cov.features(ab.VariantFeatures(alt, list(x)), is_measurement=meas)
        return cov, fs, x
    else:
        d = {"p": 1, "f": 2}.get(kind, dim)
        x, _ = gp.planted_symmetric(n, d, seed)
        if kind == "f" and n > 2:
            x[n // 2] = [1e200, 3.0]
    idv = None
    if ids:
        idv = np.arange(n, dtype=np.int64) + 7
        idv[n - 1] = idv[0]
        if n > 8:
            idv[6] = idv[2]
    return cov, features(cov, x, meas=meas, ids=idv), x


def slot_table(cov, order="program"):
    slots = [(node, param) for node, param, _ in cov.param_slots()[0]]
    if order == "reversed":
        slots = slots[::-1]
    elif order == "repeated":
        slots = slots + [slots[0]]
    return slots


def _finish(case, tree, name, family, cov, slots, seed):
    case.tree, case.name, case.family, case.cov, case.slots, case.seed = tree, name, family, cov, slots, seed
    case.nodes = plain_nodes(cov)
    case.far = tree.startswith("far:")
    return case


@functools.lru_cache(maxsize=None)
def symmetric_case(family, name, n, dim=3, order="program", ids=False, meas=True, ld_extra=3):
    """dense NLL / LOO (family 'dense_nll', 'dense_loo') and sparse mode 1 ('sparse_sym') on n points"""
    seed = _stable(f"{family}/{name}/{n}/{dim}/{order}")
    cov, fs, x = make_features(name, n, dim, seed, meas, ids)
    case = _finish(Case(), name, f"{family}:{name}:n{n}:d{fs.dim}:{order}" + (":ids" if ids else "") + ("" if meas else ":plain"),
                   family, cov, slot_table(cov, order), seed)
    rng = rng_of("w", seed)
    case.fr = case.fc = fs
    case.tr = case.tc = elevation_tangents(cov, x)
    case.ld = n + ld_extra
    case.wflat, M = padded_matrix(rng.standard_normal((n, n)), case.ld, lower=True)
    case.alpha, case.u = rng.standard_normal(n), rng.standard_normal(n)
    kind = {"dense_nll": "nll", "dense_loo": "loo", "sparse_sym": "mat"}[family]
    case.blocks = [Block(kind, 0, 0, M, True, case.alpha, case.u)]
    case.ldt = n + 2
    case.tflat = padded_tangents(case.tr, case.ldt)
    return case


@functools.lru_cache(maxsize=None)
def rect_case(name, rows, cols, dim=3, order="program", meas=(False, True), ids=None):
    """sparse mode 0: rows x cols, row and column features (and tangent columns) of their own"""
    seed = _stable(f"rect/{name}/{rows}/{cols}/{dim}/{order}/{meas}/{ids}")
    build, kind = TREES[name]
    cov = build()
    xi = yi = None
    if kind == "e":
        x, y, xi, yi, _ = planted_ids(rows, cols, dim, seed)
        fr = features(cov, x, meas=meas[0], ids=xi if ids in ("both", "rows") else None)
        fc = features(cov, y, meas=meas[1], ids=yi if ids in ("both", "cols") else None)
    else:
        _, fr, x = make_features(name, rows, dim, seed, meas[0])
        _, fc, y = make_features(name, cols, dim, seed + 1, meas[1])
    case = _finish(Case(), name, f"rect:{name}:{rows}x{cols}:d{fr.dim}:{order}:m{int(meas[0])}{int(meas[1])}:ids-{ids}", "sparse_rect", cov,
                   slot_table(cov, order), seed)
    rng = rng_of("w", seed)
    case.fr, case.fc = fr, fc
    case.tr, case.tc = elevation_tangents(cov, x), elevation_tangents(cov, y)
    case.ld = rows + 3
    case.wflat, M = padded_matrix(rng.standard_normal((rows, cols)), case.ld)
    case.blocks = [Block("mat", 0, 0, M, False)]
    case.ldtr, case.ldtc = rows + 2, cols + 5
    case.trflat, case.tcflat = padded_tangents(case.tr, case.ldtr), padded_tangents(case.tc, case.ldtc)
    return case


GROUP_SIZES = [1, 63, 64, 65, 130, 2]


@functools.lru_cache(maxsize=None)
def group_case(name, layout, dim=3, order="program", ids=False, meas=True):
    """sparse mode 2: the groups of GROUP_SIZES over one feature set.  layout 'ragged': every slab at an offset and a
    leading dimension of its own (all different, NaN between the slabs); 'uniform': every slab 130 x 130 at 130."""
    n = sum(GROUP_SIZES)
    seed = _stable(f"groups/{name}/{layout}/{dim}/{order}")
    cov, fs, x = make_features(name, n, dim, seed, meas, ids)
    case = _finish(Case(), name, f"groups:{name}:{layout}:d{fs.dim}:{order}" + (":ids" if ids else "") + ("" if meas else ":plain"), "sparse_groups", cov,
                   slot_table(cov, order), seed)
    rng = rng_of("w", seed)
    case.fr = case.fc = fs
    case.tr = case.tc = elevation_tangents(cov, x)
    case.off = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int64)
    if layout == "uniform":
        wld = [max(GROUP_SIZES)] * len(GROUP_SIZES)
        gap = 0
    else:
        wld = [s + 1 + 2 * g for g, s in enumerate(GROUP_SIZES)]
        gap = 5
    assert layout == "uniform" or len(set(wld)) == len(wld)
    woff, pos = [], 3 if gap else 0
    for s, ld in zip(GROUP_SIZES, wld):
        woff.append(pos)
        pos += ld * (max(GROUP_SIZES) if layout == "uniform" else s) + gap
    case.wflat = np.full(pos, np.nan)
    case.woff, case.wld = np.array(woff, dtype=np.int64), np.array(wld, dtype=np.int64)
    case.blocks = []
    for g, s in enumerate(GROUP_SIZES):
        view = case.wflat[woff[g]:woff[g] + wld[g] * s].reshape((wld[g], s), order="F")[:s]
        view[:] = rng.standard_normal((s, s))
        view[np.triu_indices(s, 1)] = np.nan
        case.blocks.append(Block("mat", int(case.off[g]), int(case.off[g]), view, True))
    case.ldt = n + 2
    case.tflat = padded_tangents(case.tr, case.ldt)
    return case


# ---- reference, scale, and the fp64 restatement in kernel order -----------------------------------------------------------
def _sub(fs, lo, hi):
    return ab.FeatureSet(fs.coords[lo:hi], None if fs.scales is None else list(fs.scales[lo:hi].T),
                         None if fs.eq_id is None else fs.eq_id[lo:hi], fs.is_measurement)


def block_tangents(case, b, T, mut=()):
    fr, fc = _sub(case.fr, b.rbase, b.rbase + b.nr), _sub(case.fc, b.cbase, b.cbase + b.nc)
    tr = None if case.tr is None else case.tr[b.rbase:b.rbase + b.nr]
    tc = None if case.tc is None else case.tc[b.cbase:b.cbase + b.nc]
    return eval_tangent(case.nodes, case.slots, fr, fc, tr, tc, T, mut)


def _reference(case):
    G = len(case.slots)
    ref, scale, tmax = np.zeros(G, dtype=LD), np.zeros(G, dtype=LD), 0.
    far_ok = True
    for b in case.blocks:
        dk, dka, _, tt = block_tangents(case, b, LD)
        w, wa = b.weight(LD)
        mult = b.mult().astype(LD)
        live = mult > 0
        far = live & ~(tt <= T_CAP)
        for g in range(G):
            ref[g] += np.sum(np.where(live, mult * w * dk[g], LD(0)))
            scale[g] += np.sum(np.where(live, mult * wa * dka[g], LD(0)))
            far_ok = far_ok and bool(np.all(dk[g][far] == 0) and np.all(dka[g][far] == 0))
        tmax = max(tmax, float(np.max(np.where(live & ~far, tt, 0.), initial=0.)))
        case_far = bool(far.any())
        if case_far and not case.far:
            far_ok = False
    out = (ref, scale.astype(np.float64), tmax, far_ok)
    for a in out[:2]:
        a.setflags(write=False)
    return out


_REFS = {}


def reference(case):
    """(ref (longdouble), scale, the largest exponent argument of a live pair, far pairs are exact zeros): computed once
    per case, read-only"""
    if case.name not in _REFS:
        _REFS[case.name] = _reference(case)
    return _REFS[case.name]


def kernel_order_partials(case, mut=(), phantom_tiles=0):
    """partial[tile][slot] in fp64 in the order of contract_tile and reduce_tile: a lane's 16 columns (c = wave, wave + 4, ...)
    one after the other, the butterfly over the 64 lanes, the four waves from the left.  phantom_tiles: zero partials behind
    the real ones (the tiles of a padded batch that lie wholly behind the problem).  mut: the faults of the host file."""
    G = len(case.slots)
    parts = []
    for bno, b in enumerate(case.blocks):
        dk, _, _, _ = block_tangents(case, b, np.float64, mut)
        if "wrong_ld" in mut and case.family == "sparse_groups":
            ld = int(case.wld[(bno + 1) % len(case.blocks)])
            i, j = np.arange(b.nr)[:, None], np.arange(b.nc)[None, :]
            idx = np.minimum(int(case.woff[bno]) + i + j * ld, case.wflat.size - 1)
            M = np.where(i >= j, case.wflat[idx], 0.)
            w = M
        else:
            w, _ = b.weight(np.float64)
        mult = b.mult()
        if "diag_twice" in mut and b.lower:
            mult = np.where(mult > 0, 2., 0.)
        if "strict_lower" in mut and b.lower:
            mult = np.where(mult == 2., 2., 0.)
        tiles = b.tiles(row_major="row_major" in mut)
        tr, tc = -(-b.nr // CT), -(-b.nc // CT)
        drop = None
        if "drop_row" in mut or "drop_col" in mut:  # in the last tile: its last valid row, first or last valid column
            bi, bj = tiles[-1]
            i = min(b.nr, (bi + 1) * CT) - 1
            j = bj * CT if "drop_row" in mut else min(b.nc - 1, (bj + 1) * CT - 1, i if b.lower else b.nc)
            drop = (i, j) if bno == len(case.blocks) - 1 else None
        P = np.zeros((G, tr * CT, tc * CT))
        with np.errstate(all="ignore"):
            for g in range(G):
                prod = np.where(mult > 0, (mult * w) * dk[g], 0.)
                if drop:
                    prod[drop] = 0.
                P[g, :b.nr, :b.nc] = prod
        for bi, bj in tiles:
            blk = P[:, bi * CT:(bi + 1) * CT, bj * CT:(bj + 1) * CT]
            if blk.shape[1:] != (CT, CT):  # (a tile the faulty decode puts outside the matrix)
                blk = np.zeros((G, CT, CT))
            lanes = blk.reshape(G, CT, CT // 4, 4)  # [slot, lane, k, wave]: column c = 4 k + wave
            acc = np.zeros((G, CT, 4))
            for k in range(CT // 4):
                acc = acc + lanes[:, :, k, :]
            off = 32
            lane = np.arange(CT)
            while off > 0:
                acc = acc + acc[:, lane ^ off, :]
                off //= 2
            v = acc[:, 0, 0]
            for wv in range(1, 4):
                v = v + acc[:, 0, wv]
            parts.append(v)
    parts += [np.zeros(G)] * phantom_tiles
    return np.array(parts).reshape(len(parts), G)


def reduce_partials(partial):
    """the sum of the rows of partial (tiles x slots) in the order of reduce_partials: thread t adds tiles t, t + 256, ..., then
    the tree over 256 threads"""
    tiles, G = partial.shape
    red = np.zeros((256, G))
    for t0 in range(0, tiles, 256):
        chunk = partial[t0:t0 + 256]
        red[:chunk.shape[0]] = red[:chunk.shape[0]] + chunk
    h = 128
    while h > 0:
        red[:h] = red[:h] + red[h:2 * h]
        h //= 2
    return red[0]


def kernel_order_sum(case, scale=1.0, mut=(), phantom_tiles=0):
    return scale * reduce_partials(kernel_order_partials(case, mut, phantom_tiles))


def combination(sums, which, others):
    """-1/2 S0 - S1 - 1/2 S2 as sparse_grad_reduce_kernel adds it, the contraction's sums at position `which`"""
    sets, o = [], 0
    for q in range(3):
        if q == which:
            sets.append(sums)
        else:
            sets.append(others[o]); o += 1
    total = np.zeros_like(sums)
    for q, sc in enumerate((-0.5, -1.0, -0.5)):
        total = total + sc * sets[q]
    return total


def ratio(got, ref, bound):
    """max |got - ref| / bound; inf where got is not finite"""
    got = np.asarray(got)
    if got.size == 0:
        return 0.
    if not np.all(np.isfinite(got)):
        return np.inf
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0., 0., err / bound)
    return float(np.max(r))


# ---- the input conditions ---------------------------------------------------------------------------------------------------
def check_inputs(case):
    nodes = case.nodes
    metrics = {nd["metric"] for nd in nodes if nd["op"] <= M52}
    if metrics & {capi.METRIC_RADIAL, capi.METRIC_ANGULAR}:
        for fs in (case.fr, case.fc):
            x = fs.coords
            assert x.shape[1] == 3 and np.all(x * 2 == np.round(x * 2)), case.name
            nn = (x * x).sum(axis=1)
            assert np.all(np.sqrt(nn) * 2 == np.round(np.sqrt(nn) * 2)), case.name
        seen_par = seen_anti = False
        for b in case.blocks:
            fr, fc = _sub(case.fr, b.rbase, b.rbase + b.nr), _sub(case.fc, b.cbase, b.cbase + b.nc)
            D = distances(fr, fc, metrics | {capi.METRIC_ANGULAR})
            c = D["cos"]
            x, y = fr.coords, fc.coords
            nx, ny = np.sqrt((x * x).sum(axis=1)), np.sqrt((y * y).sum(axis=1))
            parallel = np.all(x[:, None, :] * ny[None, :, None] == y[None, :, :] * nx[:, None, None], axis=2)
            anti = np.all(x[:, None, :] * ny[None, :, None] == -y[None, :, :] * nx[:, None, None], axis=2)
            assert np.all(c[parallel] == 1.) and np.all(c[anti] == -1.), case.name
            assert np.all(np.abs(c[~(parallel | anti)]) <= 0.99), case.name
            if b.lower:
                low = np.arange(b.nr)[:, None] > np.arange(b.nc)[None, :]
                seen_par, seen_anti = seen_par or bool((parallel & low).any()), seen_anti or bool((anti & low).any())
        if case.lower and case.fr.n > 8:
            assert seen_par and seen_anti, case.name
    _, scale, tmax, far_ok = reference(case)
    assert tmax <= case.t_cap <= T_CAP, (case.name, tmax, case.t_cap)
    assert far_ok, case.name
    assert np.all(np.isfinite(scale)), case.name
    if any(nd["op"] in (capi.OP_INDEPENDENT_NOISE, capi.OP_NUGGET) for nd in nodes):
        planted = False
        for b in case.blocks:
            eq = equality(_sub(case.fr, b.rbase, b.rbase + b.nr), _sub(case.fc, b.cbase, b.cbase + b.nc))
            live = b.mult() > 0
            off_diag = live & (np.arange(b.nr)[:, None] != np.arange(b.nc)[None, :]) if b.lower else live
            planted = planted or bool((eq & off_diag).any())
        if (case.lower and case.fr.n > 8) or (not case.lower and TREES[case.tree][1] == "e"):
            assert planted, case.name


# ---- the case lists ------------------------------------------------------------------------------------------------------------
N_SYM = [1, 2, 63, 64, 65, 129, 257]
N_LARGE = 1473  # 24 row tiles, 300 tiles: the strided loop of reduce_partials and lower_tile's correction loops
DIMS = [1, 2, 3, 4, 5, 8]
RECT_SHAPES = [(1, 1), (63, 65), (64, 64), (65, 129), (130, 63), (2, 193)]
SYM_FAMILIES = ["dense_nll", "dense_loo", "sparse_sym"]
# the trees every family runs at one small shape at least (the host file's faults need them there)
CORE_TREES = ["scaling", "noise*radial", "radial*noise", "m52_e+meas(noise)", "m52_e*m52_e", "far:noise*se", "variant", "ten_slots",
              "poly3+noise", "m32_r*m32_a"]


def symmetric_specs(family):
    """keyword sets of symmetric_case"""
    shift = SYM_FAMILIES.index(family)
    specs = [dict(name=nm, n=65, ids=(k + shift) % 3 == 1, meas=not (nm == "m52_e+meas(noise)" or (k + shift) % 5 == 4))
             for k, nm in enumerate(TREE_NAMES)]
    for k, n in enumerate(N_SYM):
        for j in range(3):
            nm = TREE_NAMES[(3 * k + j + 5 * shift) % len(TREE_NAMES)]
            specs.append(dict(name=nm, n=n, ids=(k + j) % 2 == 1))
        specs.append(dict(name=CORE_TREES[(k + shift) % len(CORE_TREES)], n=n))
    specs += [dict(name="m32_e+noise3", n=65, dim=d) for d in DIMS]
    specs += [dict(name="scaling", n=65, dim=d) for d in (2, 5)]
    specs += [dict(name="ten_slots", n=65, order=o) for o in ("reversed", "repeated")]
    specs += [dict(name="scaling", n=129, order=o) for o in ("reversed", "repeated")]
    specs.append(dict(name="const+noise", n=N_LARGE))
    seen, out = set(), []
    for s in specs:
        key = tuple(sorted(s.items()))
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


def rect_specs():
    specs = []
    for k, (r, c) in enumerate(RECT_SHAPES):
        for j in range(4):
            nm = TREE_NAMES[(4 * k + j) % len(TREE_NAMES)]
            specs.append(dict(name=nm, rows=r, cols=c, ids=ID_MODES[(k + j) % 4]))
        specs.append(dict(name=CORE_TREES[k % len(CORE_TREES)], rows=r, cols=c))
        specs.append(dict(name=CORE_TREES[(k + 6) % len(CORE_TREES)], rows=r, cols=c))
    specs += [dict(name=nm, rows=65, cols=129) for nm in TREE_NAMES]
    specs += [dict(name="m52_e+meas(noise)", rows=65, cols=129, meas=m, ids=ID_MODES[k]) for k, m in enumerate(gp.MEAS_COMBOS)]
    specs += [dict(name="m32_e+noise3", rows=63, cols=65, ids=i) for i in ID_MODES]
    specs += [dict(name="m32_e+noise3", rows=63, cols=65, dim=d) for d in DIMS]
    specs += [dict(name="scaling", rows=130, cols=63, order=o) for o in ("reversed", "repeated")]
    seen, out = set(), []
    for s in specs:
        key = tuple(sorted(s.items()))
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


def group_specs():
    specs = [dict(name=nm, layout=("ragged", "uniform")[k % 2], ids=k % 3 == 1) for k, nm in enumerate(TREE_NAMES)]
    specs += [dict(name=nm, layout="ragged") for nm in CORE_TREES] + [dict(name=nm, layout="uniform") for nm in CORE_TREES[:4]]
    specs += [dict(name="m32_e+noise3", layout="ragged", dim=d) for d in DIMS]
    specs += [dict(name="scaling", layout="ragged", order=o) for o in ("reversed", "repeated")]
    specs.append(dict(name="m52_e+meas(noise)", layout="ragged", meas=False))
    seen, out = set(), []
    for s in specs:
        key = tuple(sorted(s.items()))
        if key not in seen:
            seen.add(key)
            out.append(s)
    return out


# the ragged batches: (tree, n_b, dim, number of slots kept) per problem under the padded n = 192 (three tile rows: the
# third is phantom for the problems of 1 and 64 rows and partial for none)
N_PAD = 192
BATCHES = {
    "slots-0-3-9": [("m32_e+noise3", 1, 1, 0), ("m32_e+noise3", 64, 3, 3), ("nine_slots", 130, 3, 9)],
    "slots-9-0-3": [("nine_slots", 1, 3, 9), ("poly3+noise", 64, 1, 0), ("m32_e+noise3", 130, 1, 3)],
    "scaling": [("scaling", 130, 3, 6), ("scaling", 1, 1, 6), ("m32_r*m32_a", 64, 3, 5)],
    "core": [("noise*radial", 64, 3, 5), ("m52_e+meas(noise)", 130, 2, 3), ("variant", 1, 3, 7)],
    "far": [("far:noise*se", 130, 2, 4), ("const+noise", 1, 3, 2), ("far:noise*se", 64, 2, 2)],
}


def batch_problems(batch, loo):
    """the dense single-problem cases of a batch, their slot tables cut to the batch's slot counts"""
    out = []
    for name, n, dim, ns in BATCHES[batch]:
        c = symmetric_case("dense_loo" if loo else "dense_nll", name, n, dim=dim, meas=name != "m52_e+meas(noise)", ld_extra=1 + n % 3)
        assert ns <= len(c.slots)
        out.append((c, ns))
    return out


def cut_slots(case, ns):
    """`case` with the first ns slots of its table (a view: everything else is shared)"""
    import copy
    c = copy.copy(case)
    c.slots = case.slots[:ns]
    c._t_cap = case.t_cap
    c.name = f"{case.name}:first{ns}"
    return c


# ---- the debug entry points --------------------------------------------------------------------------------------------------------
_P, _PF, _I64 = C.c_void_p, C.POINTER(capi.Features), C.c_int64


@functools.lru_cache(maxsize=1)
def debug_lib():
    lib = capi.load_debug()
    lib.agp_debug_contract_dense.restype = C.c_int
    lib.agp_debug_contract_dense.argtypes = [_P, _P, _PF, C.c_int, _P, _P, _I64, _I64, C.c_int, _P, _I64, _I64, _P, _P, C.c_double, _P,
                                             _I64, _P, _I64]
    lib.agp_debug_contract_batched.restype = C.c_int
    lib.agp_debug_contract_batched.argtypes = [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _I64, C.c_double, _P,
                                               _I64, _I64, _P, _I64]
    lib.agp_debug_contract_sparse.restype = C.c_int
    lib.agp_debug_contract_sparse.argtypes = [_P, _P, _PF, _PF, C.c_int, C.c_int, _P, _P, _I64, _I64, _P, _I64, _I64, _P, _I64, _I64, _I64,
                                              _P, _P, _P, C.c_int, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _P, _I64]
    return lib


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def slot_array(slots):
    arr = (capi.GradientSlot * max(len(slots), 1))()
    for k, (node, param) in enumerate(slots):
        arr[k].node, arr[k].param = node, param
    return arr


OUT_EXTRA = 3  # canary words behind the n_slots results


def run_dense(ctx, case, loo, scale, tiles_extra=2, u=None, **override):
    """agp_debug_contract_dense: (status, out (n_slots + OUT_EXTRA, canaries behind the results), partial (tiles + tiles_extra
    rows of GRAD_GROUP, canaries behind the tiles))"""
    G = len(case.slots)
    out, partial = gp.canaries(G + OUT_EXTRA), gp.canaries((lower_tiles(case.fr.n) + tiles_extra) * GRAD_GROUP)
    u = (case.u if loo else np.full(case.fr.n, np.nan)) if u is None else u
    sx = case.fr.as_struct()
    a = dict(n_slots=G, ldt=case.ldt, tang_elems=0 if case.tflat is None else case.tflat.size, ldc=case.ld, c_elems=case.wflat.size,
             out_elems=out.size, partial_elems=partial.size)
    a.update(override)
    st = debug_lib().agp_debug_contract_dense(ctx._h, ctx.kernel(case.cov), C.byref(sx), a["n_slots"], slot_array(case.slots), _ptr(case.tflat),
                                              a["ldt"], a["tang_elems"], 1 if loo else 0, _ptr(case.wflat), a["ldc"], a["c_elems"],
                                              _ptr(case.alpha), _ptr(u), scale, _ptr(out), a["out_elems"], _ptr(partial), a["partial_elems"])
    return st, out, partial.reshape(-1, GRAD_GROUP)


def run_batched(ctx, problems, loo, scale, n_pad=N_PAD, **override):
    """agp_debug_contract_batched on [(case, slots kept)]: (status, out (count x ldo, canaries), partial ([problem][slot group]
    [tile][GRAD_GROUP], canaries), ldo, slot groups)"""
    count = len(problems)
    max_slots = max(ns for _, ns in problems)
    groups, tiles = -(-max_slots // GRAD_GROUP), lower_tiles(n_pad)
    ldo = max_slots + 2
    out = gp.canaries(ldo * count + OUT_EXTRA)
    partial = gp.canaries(max(count * groups * tiles * GRAD_GROUP, 1) + GRAD_GROUP)
    keep = []

    def ptrs(items):
        arr = (C.c_void_p * count)(*[None if a is None else a.ctypes.data for a in items])
        keep.append(items)
        return arr
    handles = [ctx.kernel(c.cov) for c, _ in problems]
    kernels = (C.c_void_p * count)(*[h.value if isinstance(h, C.c_void_p) else h for h in handles])
    structs = [c.fr.as_struct() for c, _ in problems]
    feats = (C.c_void_p * count)(*[C.addressof(s) for s in structs])
    slot_arrays = [slot_array(c.slots[:ns]) for c, ns in problems]
    slots = (C.c_void_p * count)(*[C.addressof(s) for s in slot_arrays])
    n_slots = np.array([ns for _, ns in problems], dtype=np.int32)
    us = [c.u if loo else np.full(c.fr.n, np.nan) for c, _ in problems]
    i64 = lambda v: np.array(v, dtype=np.int64)  # noqa: E731
    ldt, te = i64([c.ldt for c, _ in problems]), i64([0 if c.tflat is None else c.tflat.size for c, _ in problems])
    ldc, ce = i64([c.ld for c, _ in problems]), i64([c.wflat.size for c, _ in problems])
    a = dict(n_pad=n_pad, ldo=ldo, out_elems=out.size, partial_elems=partial.size)
    a.update(override)
    st = debug_lib().agp_debug_contract_batched(ctx._h, count, kernels, feats, _ptr(n_slots), slots, ptrs([c.tflat for c, _ in problems]),
                                                _ptr(ldt), _ptr(te), 1 if loo else 0, ptrs([c.wflat for c, _ in problems]), _ptr(ldc),
                                                _ptr(ce), ptrs([c.alpha for c, _ in problems]), ptrs(us), a["n_pad"], scale, _ptr(out),
                                                a["ldo"], a["out_elems"], _ptr(partial), a["partial_elems"])
    return st, out, partial, ldo, groups


def sparse_others(case, which):
    """the two other partial sets of the three-way combination: 3 and 300 tiles of standard normals"""
    rng = rng_of("others", case.seed, which)
    return rng.standard_normal((3, GRAD_GROUP)), rng.standard_normal((300, GRAD_GROUP))


def run_sparse(ctx, case, which=0, tiles_extra=2, **override):
    """agp_debug_contract_sparse: (status, out, combo (n_slots + OUT_EXTRA each), partial)"""
    G = len(case.slots)
    mode = {"sparse_rect": 0, "sparse_sym": 1, "sparse_groups": 2}[case.family]
    out, combo = gp.canaries(G + OUT_EXTRA), gp.canaries(G + OUT_EXTRA)
    partial = gp.canaries((case.tiles + tiles_extra) * GRAD_GROUP)
    oa, ob = sparse_others(case, which)
    sr = case.fr.as_struct()
    sc = case.fc.as_struct() if mode == 0 else None
    if mode == 0:
        trf, ldtr, tcf, ldtc = case.trflat, case.ldtr, case.tcflat, case.ldtc
    else:
        trf, ldtr, tcf, ldtc = case.tflat, case.ldt, None, 0
    off, woff, wld, Gn = (case.off, case.woff, case.wld, len(case.blocks)) if mode == 2 else (None, None, None, 0)
    a = dict(mode=mode, n_slots=G, ldtr=ldtr, tr_elems=0 if trf is None else trf.size, ldtc=ldtc, tc_elems=0 if tcf is None else tcf.size,
             ldw=0 if mode == 2 else case.ld, w_elems=case.wflat.size, G=Gn, off=off, woff=woff, wld=wld, which=which, out_elems=out.size,
             combo_elems=combo.size, partial_elems=partial.size)
    a.update(override)
    st = debug_lib().agp_debug_contract_sparse(ctx._h, ctx.kernel(case.cov), C.byref(sr), None if sc is None else C.byref(sc), a["mode"],
                                               a["n_slots"], slot_array(case.slots), _ptr(trf), a["ldtr"], a["tr_elems"], _ptr(tcf), a["ldtc"],
                                               a["tc_elems"], _ptr(case.wflat), a["ldw"], a["w_elems"], a["G"], _ptr(a["off"]),
                                               _ptr(a["woff"]), _ptr(a["wld"]), a["which"], _ptr(oa), oa.shape[0], _ptr(ob), ob.shape[0],
                                               _ptr(out), a["out_elems"], _ptr(combo), a["combo_elems"], _ptr(partial), a["partial_elems"])
    return st, out, combo, partial.reshape(-1, GRAD_GROUP)
