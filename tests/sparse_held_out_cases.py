"""Shared by tests/test_sparse_held_out_host.py and tests/test_sparse_held_out_gpu.py: the fixed problems of the sparse
model's leave-one-group-out cross validation (agp_sparse_held_out), the numpy closed form of its outputs from the dense
Kt, and the real leave-group-out refit of the dense PITC statement it must agree with."""
import numpy as np

from sparse_gradient_cases import assemble_kt

# group sizes of the four shapes: lock step with a group wider than one 128 panel | lock step, many small blocks |
# padded slabs, sizes on both sides of each power of two | one fit per block, singletons included
SHAPES = {
    "two_of_130": [130, 130],
    "64_of_4": [4] * 64,
    "ragged_13": [65, 64, 63, 33, 31, 17, 16, 9, 7, 4, 3, 2, 1],
    "ragged_35": [130, 65, 33, 17, 16, 7, 3, 2, 1] + [1] * 26,
}
LENGTH, SIGMA, NOISE = 2.5, 1.5, 0.2
MEASUREMENT_NUGGET, INDUCING_NUGGET = 1e-8, 1e-6


def problem_1d(shape, seed=5):
    """(x sorted uniform on [0, 30], y, y_var in [0.01, 0.04], offsets, 30 inducing points on a line)"""
    sizes = SHAPES[shape]
    n = int(np.sum(sizes))
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0., 30., n))
    y = np.sin(x) + 0.2 * x + 0.1 * rng.standard_normal(n)
    yvar = rng.uniform(0.01, 0.04, n)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return x, y, yvar, offsets, np.linspace(0., 30., 30)


def se(a, b, length=LENGTH, sigma=SIGMA):
    """SquaredExponential(length, sigma) of the library: sigma^2 exp(-(d / length)^2)"""
    d = np.asarray(a, dtype=np.float64)[:, None] - np.asarray(b, dtype=np.float64)[None, :]
    return sigma * sigma * np.exp(-(d / length) ** 2)


def closed_form(Kmm, Kpp, Kfu, Kuu, yvar, nugget, offsets, y):
    """The outputs of agp_sparse_held_out from the dense Kt.  Kmm: k(Measurement x, Measurement x); Kpp: k(x, x) at plain
    features; Kfu: k(x, u); Kuu: k(u, u) + inducing nugget I; yvar: the target variances (zeros for none).
    Returns a dict: per group lists mean, cov, nll_joint, nll_marginal, cond_V, and cond_Kt."""
    n = len(y)
    d = yvar + nugget
    Kt = assemble_kt(Kmm, Kfu, Kuu, d, offsets)
    Kinv = np.linalg.inv(Kt)
    alpha = Kinv @ y
    out = {"mean": [], "cov": [], "nll_joint": [], "nll_marginal": [], "cond_V": [], "cond_Kt": np.linalg.cond(Kt),
           "cond_Kuu": np.linalg.cond(Kuu)}
    for g in range(len(offsets) - 1):
        sl = slice(offsets[g], offsets[g + 1])
        sigma = np.linalg.inv(Kinv[sl, sl])
        sigma = 0.5 * (sigma + sigma.T)
        dg = sigma @ alpha[sl]
        M = Kmm[sl, sl] - Kpp[sl, sl]
        cov = sigma - np.diag(d[sl]) - M
        V = cov + np.diag(yvar[sl])
        sz = sl.stop - sl.start
        sign, logdet = np.linalg.slogdet(V)
        out["mean"].append(y[sl] - dg)
        out["cov"].append(cov)
        # (without target variances V_g is the latent covariance of close points: singular to working precision)
        out["nll_joint"].append(0.5 * (logdet + dg @ np.linalg.solve(V, dg) + sz * np.log(2 * np.pi)) if sign > 0 else np.nan)
        v = np.diag(V)
        out["nll_marginal"].append(0.5 * np.sum(np.log(v) + dg * dg / v + np.log(2 * np.pi)))
        out["cond_V"].append(np.linalg.cond(V))
    assert n == offsets[-1]
    return out


def refit_prediction(Kmm, Kpp, Kfu, Kuu, yvar, nugget, offsets, y, g):
    """fit(all groups but g).predict(x_g) of the dense PITC statement the way the reference makes it (sparse_gp.hpp:
    _fit_impl :354-381, _predict_impl :447-521): A = blockdiag(K_ff + D - Q_ff) = L_A L_A^T, K_uu = L_u L_u^T, the QR of
    B = [L_A^-1 K_fu; L_u^T] (B^T B = Sigma^-1), v the least-squares solution of B v = [L_A^-1 y; 0]; then at the plain
    features of g: mean = K_*u v, covariance = K_** - |L_u^-1 K_u*|^2 + |R^-T K_u*|^2.  Square roots throughout: the
    conditioning is that of B, not of Sigma^-1."""
    n = len(y)
    held = np.zeros(n, dtype=bool)
    held[offsets[g]:offsets[g + 1]] = True
    rest = ~held
    d = yvar + nugget
    Lu = np.linalg.cholesky(Kuu)
    P = np.linalg.solve(Lu, Kfu.T)  # L_u^-1 K_uf
    rows, yw = [], []
    for h in range(len(offsets) - 1):
        if h == g:
            continue
        sl = slice(offsets[h], offsets[h + 1])
        La = np.linalg.cholesky(Kmm[sl, sl] + np.diag(d[sl]) - P[:, sl].T @ P[:, sl])
        rows.append(np.linalg.solve(La, Kfu[sl]))
        yw.append(np.linalg.solve(La, y[sl]))
    B = np.vstack(rows + [Lu.T])
    rhs = np.concatenate(yw + [np.zeros(Kuu.shape[0])])
    Qb, R = np.linalg.qr(B)
    v = np.linalg.solve(R, Qb.T @ rhs)
    Ks = Kfu[held]
    Q_sqrt = P[:, held]
    S_sqrt = np.linalg.solve(R.T, Ks.T)
    return Ks @ v, Kpp[np.ix_(held, held)] - Q_sqrt.T @ Q_sqrt + S_sqrt.T @ S_sqrt
