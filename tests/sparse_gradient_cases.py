"""Shared by tests/test_sparse_gradient_host.py, tests/test_sparse_gradient_gpu.py and scripts/record_sparse_golden.py:
the two fixed sparse-GP problems whose agp_sparse_nll / agp_sparse_fit_create outputs are pinned in
tests/golden/sparse_fit_parent.json (recorded before agp_sparse_nll_gradient existed), and the numpy restatement of the
structured gradient formulas (include/albatross_amd.h, agp_sparse_nll_gradient)."""
import numpy as np


def golden_problem(which):
    """(covariance, features, targets, target variances, group keys, inducing points, measurement nugget, inducing nugget)"""
    import albatross_amd as ab
    if which == "uniform_1d":  # equal groups of 128: the lock-step path
        rng = np.random.default_rng(7)
        n, gs, m = 512, 128, 30
        x = np.sort(rng.uniform(0., 30., n))
        y = np.sin(x) + 0.2 * x + 0.1 * rng.standard_normal(n)
        yvar = rng.uniform(0.01, 0.04, n)
        cov = ab.SquaredExponential(2.5, 1.5) + ab.measurement_only(ab.IndependentNoise(0.2))
        keys = np.arange(n) // gs
        return cov, x, y, yvar, keys, np.linspace(0., 30., m), 1e-8, 1e-6
    if which == "ragged_3d":  # interval groups of comparable size: the padded lock-step path
        rng = np.random.default_rng(11)
        n, m = 900, 130
        x = rng.uniform(0., 20., (n, 3))
        y = np.sin(x[:, 0]) + 0.3 * x[:, 0] + 0.1 * rng.standard_normal(n)
        cov = ab.Matern52(4.0, 2.0) + ab.measurement_only(ab.IndependentNoise(0.2))
        keys = np.floor(x[:, 0] / 1.7).astype(np.int64)
        return cov, x, y, None, keys, rng.uniform(0., 20., (m, 3)), 1e-10, 1e-6
    raise KeyError(which)


def golden_model(which, ctx):
    import albatross_amd as ab
    cov, x, y, yvar, keys, u, mn, inn = golden_problem(which)
    lookup = {np.asarray(f, dtype=np.float64).tobytes(): int(k) for f, k in zip(x, keys)}
    grouper = lambda f: lookup[np.asarray(f, dtype=np.float64).tobytes()]
    model = ab.sparse_gp_from_covariance(cov, grouper, ab.FixedInducingPoints(u), "sparse", context=ctx)
    model.set_param("measurement_nugget", mn)
    model.set_param("inducing_nugget", inn)
    targets = y if yvar is None else ab.MarginalDistribution(y, yvar)
    return model, ab.RegressionDataset(x, targets)


# ---- numpy restatement of the sparse likelihood and of its gradient ------------------------------------------------
def block_mask(offsets, n):
    """n x n boolean: True inside the group blocks"""
    group = np.searchsorted(np.asarray(offsets)[1:], np.arange(n), side="right")
    return group[:, None] == group[None, :]


def assemble_kt(Kff, Kfu, Kuu, d, offsets):
    """Kt = A + Q of the sparse model: Q = K_fu K_uu^-1 K_uf, A = bd(K_ff + diag(d) - Q)"""
    Q = Kfu @ np.linalg.solve(Kuu, Kfu.T)
    return Q + np.where(block_mask(offsets, len(d)), Kff + np.diag(d) - Q, 0.)


def dense_nll(Kt, y):
    sign, logdet = np.linalg.slogdet(Kt)
    return 0.5 * (logdet + y @ np.linalg.solve(Kt, y) + len(y) * np.log(2 * np.pi))


def assemble_dkt(Kfu, Kuu, offsets, dKff, dKfu, dKuu, dd):
    """d Kt for given derivatives of K_ff, K_fu, K_uu (nugget included) and of the diagonal d"""
    E = np.linalg.solve(Kuu, Kfu.T).T
    dQ = dKfu @ E.T + E @ dKfu.T - E @ dKuu @ E.T
    return dQ + np.where(block_mask(offsets, Kfu.shape[0]), dKff + np.diag(dd) - dQ, 0.)


def dense_gradient(Kt, y, dKt):
    """the plain dense formula 1/2 <Kt^-1 - alpha alpha^T, dKt>"""
    Kinv = np.linalg.inv(Kt)
    alpha = Kinv @ y
    return 0.5 * np.sum((Kinv - np.outer(alpha, alpha)) * dKt)


def structured_weights(Kff, Kfu, Kuu, d, offsets, y):
    """(bd(G) as an n x n array that is zero outside the blocks, W_fu, W_uu, alpha) through A, Sigma and V only - the
    formulas of agp_sparse_nll_gradient; no n x n inverse of Kt"""
    n, m = Kfu.shape
    Lu = np.linalg.cholesky(Kuu)
    P = np.linalg.solve(Lu, Kfu.T)                      # L_u^-1 K_uf
    E = np.linalg.solve(Lu.T, P).T                      # K_fu K_uu^-1
    Ainv = np.zeros((n, n))
    for g in range(len(offsets) - 1):
        sl = slice(offsets[g], offsets[g + 1])
        Ag = Kff[sl, sl] + np.diag(d[sl]) - P[:, sl].T @ P[:, sl]
        Ainv[sl, sl] = np.linalg.inv(Ag)
    S = Kuu + Kfu.T @ Ainv @ Kfu                        # Sigma^-1
    Lacc = np.linalg.cholesky(S)
    v = np.linalg.solve(S, Kfu.T @ (Ainv @ y))          # the information vector
    alpha = Ainv @ (y - Kfu @ v)
    V = np.linalg.solve(Lacc, Kfu.T @ Ainv).T           # A^-1 K_fu Lacc^-T
    mask = block_mask(offsets, n)
    bdG = np.where(mask, Ainv - V @ V.T - np.outer(alpha, alpha), 0.)
    KtinvE = V @ np.linalg.solve(Lacc, np.eye(m))       # A^-1 K_fu Sigma
    GE = KtinvE - np.outer(alpha, alpha @ E)
    HE = GE - bdG @ E
    return bdG, 2. * HE, -E.T @ HE, alpha


def structured_gradient(weights, dKff, dKfu, dKuu, dd):
    """(dNLL / dtheta, s_p): the three contractions and the sum of the absolute values of their terms"""
    bdG, Wfu, Wuu, _ = weights
    dA = dKff + np.diag(dd)
    g = 0.5 * (np.sum(bdG * dA) + np.sum(Wfu * dKfu) + np.sum(Wuu * dKuu))
    s = 0.5 * (np.sum(np.abs(bdG * dA)) + np.sum(np.abs(Wfu * dKfu)) + np.sum(np.abs(Wuu * dKuu)))
    return g, s
