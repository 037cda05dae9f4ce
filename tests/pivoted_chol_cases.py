"""Shared by tests/test_pivoted_chol_host.py, tests/test_pivoted_chol_gpu.py and tests/test_greedy_inducing_gpu.py: the
shapes, inputs and bounds of the greedy pivoted Cholesky factorisation (csrc/pivoted_chol.hip, agp_pivoted_cholesky)
and a numpy restatement of its definition, parameterised by dtype (float64, np.longdouble).

Definition (include/albatross_amd.h).  d_i = K_ii, d0 = max_i d_i; step j: p_j = the unselected index with the largest d
(the lowest index on equal values); stop with rank = j if d_{p_j} <= rel_tol d0 or d_{p_j} <= 0; otherwise
c_i = K_{i p_j} - sum_{t<j} L_it L_{p_j t} (t = 0, 1, ...), L_ij = c_i / sqrt(d_{p_j}), d_i = max(d_i - L_ij^2, 0), and
exactly L_{p_j j} = sqrt(d_{p_j}), d_{p_j} = 0, L_ij = 0 for rows selected before.

Pivots are NOT compared with a free-running reference: on 1000 uniform points in [0, 10]^3 with a squared exponential
kernel (l = 2) the float64 and the longdouble run of the restatement agree on 4 of 300 pivots - near-ties are decided
by the last bit.  What is checked instead (`check` below) is the output itself against the matrix K, everything
recomputed in longdouble from the returned L.  With u = 2^-53, Kmax = max_i K_ii:

  * pivot rule.  d(j)_i = K_ii - sum_{t<j} L_it^2.  p_j is unselected and d(j)_{p_j} >= max over the unselected of d(j)
    - (j + 1)^2 u Kmax.  The slack is the accumulated rounding of j subtractions of L^2, each carrying the error of a
    length-j dot product: |L_ij| <= sqrt(d_{p_j}) bounds c_i by sqrt(d_{p_j}) sqrt(K_ii), so the small pivot cancels
    out of the error of L_ij^2 and (j + 1) u Kmax per subtraction remains.  Where the values are bitwise equal the
    lower index must win exactly (the `ties` case: a constant diagonal at step 0, p_0 = 0).
  * structure.  L_{p_j j} > 0, L_{p_t j} = 0 exactly for t < j, residual_diag[p_j] = 0 exactly, residual_diag >= 0.
  * pivot rows reproduce K componentwise: |K_{p i} - sum_t L_pt L_it| <= (rank + 2) u sqrt(K_pp K_ii) for every pivot
    p and every i - the Cholesky backward bound (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3, with
    gamma_{rank+1} and the rounding of K itself), free of conditioning.
  * residual.  |residual_diag_i - (K_ii - sum_t L_it^2)| <= (rank + 1)^2 u Kmax (same derivation as the slack), and
    trace_residual within n times that of their sum.
  * stop rule.  rank < max_rank only if max residual_diag <= rel_tol d0 (or <= 0); every accepted pivot had
    d > rel_tol d0, i.e. L_{p_j j}^2 >= rel_tol d0 (1 - 4 u) (the root and its square round once each).

tests/test_pivoted_chol_host.py shows that the float64 restatement meets each of these on the very inputs of the GPU
tests (worst measured fractions of the bounds are in its docstring), and that the `duplicates` cases have exactly the
rank claimed.

Shapes come from the kernel's constants: TILE rows per workgroup (two per lane of its one wave), UNROLL columns per
trip of the t loop, CHUNK columns of the pivot's row staged in LDS at a time, THREADS entries of the partials table per
pass of the argmax (more than THREADS workgroups: `two_level`).
"""
import functools

import numpy as np

import albatross_amd as ab

U = 2.0 ** -53
TILE = 128     # csrc/pivoted_chol.hip: PC_TILE
UNROLL = 8     # PC_UNROLL
CHUNK = 512    # PC_CHUNK
THREADS = 64   # PC_THREADS
HOST_LOOK = 64  # PC_HOST_LOOK


class _Ramp(ab.ScalingFunction):
    """f(x) = 1 + 0.1 x_0: a ScalingTerm that varies over the points"""

    def get_name(self):
        return "ramp"

    def _call_impl(self, coords):
        return 1. + 0.1 * np.asarray(coords)[:, 0]


def _uniform(n, dim, seed):
    return np.random.default_rng(seed).uniform(0., 10., (n, dim))


def _se(l=2.):
    return lambda: ab.SquaredExponential(l, 1.)


# name -> (n, dim, covariance factory, max_rank, rel_tol, feature maker or None)
def _cases():
    c = {}
    # row-tile edges (Euclidean squared exponential on 3-D points: the radial fast path)
    for n in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        c[f"rows{n}"] = (n, 3, _se(), min(n, 24), 0., None)
    c["rows1000"] = (1000, 3, _se(), 40, 0., None)
    # unroll edges of the t loop
    for m in (1, UNROLL - 1, UNROLL, UNROLL + 1, 64, 65):
        c[f"rank{m}"] = (TILE + 1, 3, lambda: ab.Matern32(3., 1.3), m, 0., None)
    # across the chunk edge of the pivot-row staging and nine looks of the host: all 600 steps run
    c["chunk600"] = (1000, 3, lambda: ab.Exponential(5., 1.), CHUNK + 88, 0., None)
    # more workgroups than one pass of the argmax over the partials table
    c["two_level"] = (TILE * (THREADS + 1) + 1, 2, _se(1.5), 4, 0., None)
    # dimensions 1 and 5 (padded to 8); 3 is everywhere else
    c["dim1"] = (300, 1, lambda: ab.Matern32(1.5, 1.), 33, 0., None)
    c["dim5"] = (300, 5, lambda: ab.SquaredExponential(6., 2.), 33, 0., None)
    # the other evaluators: angular metric, a ScalingTerm product, IndependentNoise with equality ids
    c["angular"] = (300, 3, lambda: ab.Exponential(0.7, 1., ab.AngularDistance()), 33, 0.,
                    lambda: _uniform(300, 3, 41) - 5.)
    c["scaling"] = (300, 2, lambda: ab.ScalingTerm(_Ramp()) * ab.SquaredExponential(3., 1.) + ab.Constant(0.5), 33, 0., None)

    def with_ids():
        rng = np.random.default_rng(43)
        x = rng.uniform(0., 10., (300, 2))
        x[200:] = x[:100]  # the same coordinates under another id: the noise term tells them apart
        return ab.FeatureSet(x, eq_id=np.arange(300, dtype=np.int64) + 7)
    c["noise_ids"] = (300, 2, lambda: ab.SquaredExponential(3., 1.) + ab.IndependentNoise(0.3), 240, 0., with_ids)
    # a constant diagonal: step 0 is a tie of all n values, the lowest index wins
    c["ties"] = (TILE + 1, 3, _se(), 1, 0., None)
    # early stop: 1000 points in 1-D, squared exponential (l = 1): the float64 restatement stops at rank 34 of 128
    c["early_stop"] = (1000, 1, _se(1.), 128, 1e-8, None)

    # duplicates: 200 distinct points plus 100 copies, shuffled: the rank must be exactly 200
    def dup():
        rng = np.random.default_rng(47)
        base = rng.uniform(0., 10., (200, 3))
        x = np.concatenate([base, base[rng.integers(0, 200, 100)]])
        return x[rng.permutation(300)]
    c["duplicates_exp"] = (300, 3, lambda: ab.Exponential(5., 1.), 300, 1e-12, dup)
    c["duplicates_m32"] = (300, 3, lambda: ab.Matern32(3., 1.), 300, 1e-12, dup)
    return c


CASES = _cases()
DUPLICATE_RANK = 200
BIG = ("two_level",)  # K is never formed: its diagonal and its pivot rows come from blocks


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(covariance function, features: an n x dim array or a FeatureSet) of a case; never modified"""
    n, dim, cov, _, _, maker = CASES[name]
    x = maker() if maker else _uniform(n, dim, 1000 + sum(map(ord, name)))
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    return cov(), x


def coords_of(x):
    return x.coords if isinstance(x, ab.FeatureSet) else x


def subset(x, idx):
    """features idx of x, as the same kind of object"""
    if isinstance(x, ab.FeatureSet):
        return ab.FeatureSet(x.coords[idx], None, None if x.eq_id is None else x.eq_id[idx], x.is_measurement)
    return x[idx]


def gram_parts(gram, name, pivots):
    """(diagonal of K, K[pivots, :]) of a case from gram(cov, xs[, ys]); the big case block by block"""
    cov, x = inputs(name)
    n = CASES[name][0]
    if name not in BIG:
        K = gram(cov, x)
        return np.diag(K).copy(), K[np.asarray(pivots, dtype=np.int64), :], K
    diag = np.empty(n)
    for o in range(0, n, 512):
        idx = np.arange(o, min(o + 512, n))
        diag[idx] = np.diag(gram(cov, subset(x, idx)))
    rows = gram(cov, subset(x, np.asarray(pivots, dtype=np.int64)), x) if len(pivots) else np.empty((0, n))
    return diag, rows, None


def restatement(kdiag, kcol, max_rank, rel_tol, dtype=np.float64):
    """the definition in numpy; kcol(p) = column p of K.  Returns (pivots, rank, L (n x rank), d, trace)."""
    d = np.asarray(kdiag).astype(dtype)
    n = d.shape[0]
    L = np.zeros((n, max_rank), dtype=dtype)
    sel = np.zeros(n, dtype=bool)
    pivots = []
    d0 = d.max()
    tol = dtype(rel_tol)
    for j in range(max_rank):
        cand = np.where(sel, dtype(-1), d)
        p = int(np.argmax(cand))  # the first index of the maximum
        dp = cand[p]
        if dp <= tol * d0 or dp <= 0:
            break
        s = np.zeros(n, dtype=dtype)
        for t in range(j):  # the fixed order t = 0, 1, ...
            s += L[:, t] * L[p, t]
        root = np.sqrt(dp)
        col = (np.asarray(kcol(p)).astype(dtype) - s) / root
        col[sel] = 0
        col[p] = root
        dn = np.maximum(d - col * col, dtype(0))
        dn[sel] = 0
        dn[p] = 0
        L[:, j] = col
        d = dn
        sel[p] = True
        pivots.append(p)
    r = len(pivots)
    return np.asarray(pivots, dtype=np.int64), r, L[:, :r], d, d.sum()


def check(kdiag, krows, max_rank, rel_tol, pivots, rank, L, resid, trace):
    """Every bound of the module docstring, recomputed in longdouble from the returned L.  krows = K[pivots, :].
    Returns the worst measured fraction of each bound."""
    LD = np.longdouble
    n = kdiag.shape[0]
    pivots = np.asarray(pivots, dtype=np.int64)
    assert 0 <= rank <= max_rank and pivots.shape == (rank,) and L.shape == (n, rank)
    assert resid.shape == (n,)
    kd = kdiag.astype(LD)
    kmax = kd.max()
    d0 = float(kdiag.max())
    Ll = L.astype(LD)
    worst = {"pivot": 0., "rows": 0., "resid": 0., "trace": 0.}
    # pivot rule and structure
    assert len(set(pivots.tolist())) == rank, "a pivot was selected twice"
    sel = np.zeros(n, dtype=bool)
    dj = kd.copy()
    for j in range(rank):
        p = int(pivots[j])
        assert 0 <= p < n and not sel[p]
        cand = np.where(sel, LD(-1), dj)
        mx = cand.max()
        slack = LD((j + 1) ** 2) * LD(U) * kmax
        assert dj[p] >= mx - slack, f"step {j}: pivot {p} has d {dj[p]}, the maximum is {mx} (slack {slack})"
        worst["pivot"] = max(worst["pivot"], float((mx - dj[p]) / slack))
        assert L[p, j] > 0., f"L[p_{j}, {j}] = {L[p, j]}"
        assert not np.any(L[pivots[:j], j] != 0.), f"column {j} is not exactly zero on the rows selected before"
        assert float(L[p, j]) ** 2 >= rel_tol * d0 * (1. - 4. * U) and L[p, j] > 0., f"step {j} accepted a pivot under the threshold"
        sel[p] = True
        dj = dj - Ll[:, j] * Ll[:, j]
    assert not np.any(resid[pivots] != 0.), "residual_diag is not exactly zero at a pivot"
    assert np.all(resid >= 0.)
    # pivot rows reproduce K
    if rank:
        got = Ll[pivots, :] @ Ll.T
        scale = np.sqrt(kd[pivots][:, None] * kd[None, :])
        bound = LD(rank + 2) * LD(U) * scale
        err = np.abs(krows.astype(LD) - got)
        assert np.all(err <= bound), f"pivot rows: worst {float((err / bound).max()):.3g} of the bound"
        worst["rows"] = float((err / bound).max())
    # residual and trace
    rb = LD((rank + 1) ** 2) * LD(U) * kmax
    err = np.abs(resid.astype(LD) - dj)
    assert np.all(err <= rb), f"residual: worst {float(err.max() / rb):.3g} of the bound"
    worst["resid"] = float(err.max() / rb)
    terr = abs(LD(trace) - resid.astype(LD).sum())
    assert terr <= n * rb, f"trace: {float(terr / (n * rb)):.3g} of the bound"
    worst["trace"] = float(terr / (n * rb))
    # stop rule
    if rank < max_rank:
        assert resid.max() <= rel_tol * d0 or resid.max() <= 0., f"stopped at rank {rank} with residual {resid.max()} (d0 {d0})"
    return worst
