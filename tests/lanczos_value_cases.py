"""Shared by tests/test_lanczos_quadrature_host.py and tests/test_iterative_value_gpu.py: the shapes, the seeds and a float64
numpy restatement of the log-likelihood VALUE of the matrix-free fit (csrc/iterative.hip: agp_iterative_nll;
csrc/lanczos_quadrature.h).  Nothing here is measured.

The definition restated here (A, L, m, delta, P = L L^T + delta I those of tests/iterative_fit_cases.py):
    log det A = log det P + tr log(M),  M = P^-1/2 A P^-1/2,  log det P = (n - m) log delta + log det(delta I + L^T L)
    z ~ N(0, P):  E[u^T log(M) u] = tr log M for u = P^-1/2 z.  Preconditioned CG on A x = z is Lanczos on M started at u;
    with a_k, b_k the alpha and beta of iteration k (b_0 = 0):
        T[k, k] = 1 / a_k + b_k / a_{k-1},   T[k-1, k] = T[k, k-1] = sqrt(b_k) / a_{k-1}
        s = rz_0 sum_i V[0, i]^2 log lambda_i,  (lambda, V) = eigh(T),  rz_0 = z^T P^-1 z
    log det A ~ log det P + mean_c s_c,  stderr = sqrt(sum (s_c - mean)^2 / (t (t - 1))),
    NLL = 1/2 alpha^T A alpha + 1/2 log det A + n/2 log 2 pi
    gradient from the same solves: s_cp = w_c^T dA_p v_c with w = A^-1 z, v = P^-1 z.
Probes: the caller's, or z = L g1 + sqrt(delta) g2 with g2 = agp_standard_normal(seed) on n rows and g1 =
agp_standard_normal(seed ^ FACTOR_SEED) on m rows, column c of both for probe c.

Bars:
  * quadrature entry against eigh of the same T: 1e-12 rz_0 max|log lambda| (QUADRATURE_BAR).
  * exhausting probes Z = sqrt(t) [L | sqrt(delta) I], t = n + m (Z Z^T / t = P: the mean is exact) at a fit tolerance of
    1e-12: |log det - dense| and |value - dense| <= 1e-8 (n + |dense|), the project's bar for iterative against dense.
  * seeded samples: 1e-8 of the sample's scale rz_0 max|log lambda| (value) and sum |w_i| |dA_ij| |v_j| (gradient).
  * the seeded estimate: at most 4 of its own standard errors from the dense value; the seed below is one for which this
    restatement is under 2 (asserted by the host test).
"""
import functools
import math

import numpy as np

import gram_tangent_cases as tc
import iterative_fit_cases as ic
import prediction_score_cases as ps

FIT_TOL = 1e-12
QUADRATURE_BAR = 1e-12
PARITY = 1e-8
SAMPLE_BAR = 1e-8
FACTOR_SEED = 0x9E3779B97F4A7C15  # pcg_probe_factor_seed, csrc/iterative_internal.h

EXACT_SHAPES = [("n65_3d", 0), ("n65_3d", 16), ("n130_3d", 64)]  # (inputs of gram_tangent_cases, preconditioner rank)
ESTIMATE = ("n777_2d", 64, 64, 3)  # (inputs, rank, probes, seed)
PROBE_N = [1, 255, 256, 257, 777]
PROBE_M = [0, 1, 64]
PROBE_T = [1, 16, 17]
MUTATIONS = ("shift_b", "drop_rz0", "no_sqrt")


@functools.lru_cache(maxsize=None)
def preconditioner(name, rank):
    A, _, _ = tc.dense_system(name)
    return ic.Preconditioner(A, rank)


def preconditioner_from(L, delta):
    """the restated preconditioner around a factor and a delta that were downloaded from a live fit"""
    P = ic.Preconditioner.__new__(ic.Preconditioner)
    P.n, P.rank = L.shape
    P.L, P.delta = L, float(delta)
    if P.rank:
        P.chol = np.linalg.cholesky(P.delta * np.eye(P.rank) + L.T @ L)
    return P


def log_det_p(P):
    out = (P.n - P.rank) * math.log(P.delta)
    if P.rank:
        out += 2. * float(np.log(np.diag(P.chol)).sum())
    return out


def pcg_coefficients(A, P, z, tol=FIT_TOL, max_iterations=1000, steps=None):
    """(rz_0, a[k], b[k], x): the recurrence of iterative_fit_cases.pcg for one right-hand side with its coefficients kept;
    `steps`: that many iterations whatever the residual"""
    n = A.shape[0]
    x, r = np.zeros(n), z.copy()
    bnorm = math.sqrt(float(z @ z))
    a, b = [], []
    p, rz_old, rz0 = None, 0., 0.
    for k in range(steps if steps is not None else max_iterations):
        zz = P.apply(r)
        rz = float(r @ zz)
        beta = 0. if k == 0 else rz / rz_old
        if k == 0:
            rz0 = rz
        p = zz if k == 0 else zz + beta * p
        q = A @ p
        alpha = rz / float(p @ q)
        x = x + alpha * p
        r = r - alpha * q
        rz_old = rz
        a.append(alpha)
        b.append(beta)
        if steps is None and math.sqrt(float(r @ r)) <= tol * bnorm:
            break
    else:
        assert steps is not None, "not converged"
    return rz0, np.array(a), np.array(b), x


def tridiagonal(a, b, mutation=None):
    k = len(a)
    T = np.zeros((k, k))
    bb = np.array(b, dtype=np.float64)
    if mutation == "shift_b":  # b_k read one row late
        bb = np.concatenate([[0.], bb[:-1]])
    for i in range(k):
        T[i, i] = 1. / a[i] + (bb[i] / a[i - 1] if i else 0.)
        if i:
            T[i - 1, i] = T[i, i - 1] = (bb[i] if mutation == "no_sqrt" else math.sqrt(bb[i])) / a[i - 1]
    return T


def quadrature(rz0, a, b, mutation=None):
    """(rz_0 e_1^T log(T) e_1 by eigh, its scale rz_0 max|log lambda|)"""
    lam, V = np.linalg.eigh(tridiagonal(a, b, mutation))
    w = V[0] ** 2
    scale = (1. if mutation == "drop_rz0" else rz0)
    with np.errstate(invalid="ignore"):  # (a planted defect can leave T indefinite: NaN)
        return scale * float((w * np.log(lam)).sum()), rz0 * float(np.abs(np.log(lam)).max())


def exhausting_probes(L, delta):
    """sqrt(t) [L | sqrt(delta) I], t = n + m: Z Z^T / t = L L^T + delta I"""
    n, m = L.shape
    return math.sqrt(n + m) * np.concatenate([L, math.sqrt(delta) * np.eye(n)], axis=1)


def normals(seed, n, m, t):
    """(G1 m x t, G2 n x t) of the documented probes"""
    g2 = ps.standard_normal(seed, n, 0, t)
    g1 = ps.standard_normal(seed ^ FACTOR_SEED, m, 0, t) if m else np.zeros((0, t))
    return g1, g2


def seeded_probes(seed, L, delta, t):
    g1, g2 = normals(seed, L.shape[0], L.shape[1], t)
    return L @ g1 + math.sqrt(delta) * g2


def probe_reference(L, delta, g1, g2):
    """(L g1 + sqrt(delta) g2 in longdouble, its componentwise bound gamma(m + 2) (|L| |g1| + sqrt(delta) |g2|)): m products
    and m additions in order, the product with sqrt(delta) (itself one rounding) and the last addition"""
    LD = np.longdouble
    m = L.shape[1]
    sd = math.sqrt(delta)
    want = L.astype(LD) @ g1.astype(LD) + LD(sd) * g2.astype(LD)
    size = np.abs(L) @ np.abs(g1) + sd * np.abs(g2)
    u = 2. ** -53
    g = (m + 2) * u / (1. - (m + 2) * u)
    return want, g * size


def value_restated(name, rank, Z, tol=FIT_TOL, mutation=None, P=None):
    """dict(log_det, log_det_stderr, samples, scales, nll, nll_stderr, iterations) of the definition above in numpy"""
    A, _, alpha = tc.dense_system(name)
    P = P or preconditioner(name, rank)
    n, t = A.shape[0], Z.shape[1]
    s, sc, its = np.zeros(t), np.zeros(t), np.zeros(t, dtype=int)
    for c in range(t):
        rz0, a, b, _ = pcg_coefficients(A, P, Z[:, c], tol)
        s[c], sc[c] = quadrature(rz0, a, b, mutation)
        its[c] = len(a)
    mean = s.sum() / t
    se = math.sqrt(((s - mean) ** 2).sum() / (t * (t - 1))) if t > 1 else float("nan")
    ld = log_det_p(P) + mean
    nll = 0.5 * float(alpha @ (A @ alpha)) + 0.5 * ld + 0.5 * n * math.log(2. * math.pi)
    return dict(log_det=ld, log_det_stderr=se, samples=s, scales=sc, nll=nll, nll_stderr=0.5 * se, iterations=its)


def exact_samples(name, P, Z):
    """u^T log(M) u per column from the dense eigendecomposition: with P = C C^T, M' = C^-1 A C^-T is M in another
    orthonormal basis and u' = C^-1 z the same vector there"""
    A, _, _ = tc.dense_system(name)
    n = A.shape[0]
    Pm = P.L @ P.L.T + P.delta * np.eye(n)
    C = np.linalg.cholesky(Pm)
    Ci = np.linalg.inv(C)
    lam, Q = np.linalg.eigh(Ci @ A @ Ci.T)
    U = Q.T @ (Ci @ Z)
    return (U ** 2 * np.log(lam)[:, None]).sum(axis=0)


def gradient_samples_restated(name, P, Z):
    """({name: s_cp}, {name: scale}) with an exact solve: s_cp = (A^-1 z_c)^T dA_p (P^-1 z_c)"""
    A, dA, _ = tc.dense_system(name)
    W = np.linalg.solve(A, Z)
    V = np.stack([P.apply(Z[:, c]) for c in range(Z.shape[1])], axis=1)
    samples, scales = {}, {}
    for nm, d in dA.items():
        samples[nm] = np.sum(W * (d @ V), axis=0)
        scales[nm] = np.sum(np.abs(W) * (np.abs(d) @ np.abs(V)), axis=0)
    return samples, scales


@functools.lru_cache(maxsize=None)
def dense_values(name):
    """(log det A, NLL) of the dense system in numpy"""
    A, _, alpha = tc.dense_system(name)
    n = A.shape[0]
    sign, ld = np.linalg.slogdet(A)
    assert sign > 0
    return float(ld), 0.5 * float(alpha @ (A @ alpha)) + 0.5 * float(ld) + 0.5 * n * math.log(2. * math.pi)


def parity_bar(n, dense):
    return PARITY * (n + abs(dense))


# ---- coefficient sets for the quadrature entry ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coefficient_sets():
    """[(label, rz_0, a, b)]: k = 1, 2, 3, 30, 343 iterations of the plain (rank 0) recurrence on n777_2d for one seeded probe
    - 343 runs on past convergence, where the Lanczos vectors have lost their orthogonality and T carries ghost copies - and
    one synthetic set whose 20 eigenvalues lie within 1e-5 of 4 (near 1 the scale rz_0 max|log lambda| would itself vanish
    and no float64 eigh could serve as the reference)"""
    name = ESTIMATE[0]
    A, _, _ = tc.dense_system(name)
    P = preconditioner(name, 0)
    z = seeded_probes(11, P.L, P.delta, 1)[:, 0]
    out = []
    for k in (1, 2, 3, 30, 343):
        rz0, a, b, _ = pcg_coefficients(A, P, z, steps=k)
        out.append((f"k{k}", rz0, a, b))
    out.append(("clustered", 3.5, np.full(20, 0.25), np.concatenate([[0.], np.full(19, 1e-12)])))
    return out
