"""The host quadrature of the matrix-free fit's log-likelihood value without a GPU: agp_debug_lanczos_quadrature
(csrc/lanczos_quadrature.h through csrc/debug_api.hip) against numpy's eigh of the same tridiagonal on coefficient sets the
restated recurrence records, the restatement of tests/lanczos_value_cases.py against every bound the GPU file holds the device
to, and three planted defects that miss them: b_k read one row late, rz_0 dropped, the off-diagonal without its square
root."""
import ctypes as C
import math

import numpy as np
import pytest

from albatross_amd import _capi as capi
import gram_tangent_cases as tc
import lanczos_value_cases as lv


def _p(a):
    return C.c_void_p(a.ctypes.data)


def entry(rz0, a, b):
    """(status, value) of agp_debug_lanczos_quadrature"""
    fn = capi.load_debug().agp_debug_lanczos_quadrature
    fn.restype = C.c_int
    fn.argtypes = [C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    out = np.full(1, -7.5)
    st = fn(float(rz0), _p(a), _p(b), len(a), _p(out))
    return st, float(out[0])


@pytest.mark.parametrize("which", range(6))
def test_entry_matches_eigh(which):
    label, rz0, a, b = lv.coefficient_sets()[which]
    st, got = entry(rz0, a, b)
    want, scale = lv.quadrature(rz0, a, b)
    lam = np.linalg.eigvalsh(lv.tridiagonal(a, b))
    print(f"{label}: k {len(a)}, eigenvalues {lam.min():.3g} .. {lam.max():.3g}, value {got:.12g}, "
          f"|entry - eigh| {abs(got - want) / scale:.3g} of rz0 max|log lambda|")
    assert st == capi.AGP_OK
    assert abs(got - want) <= lv.QUADRATURE_BAR * scale, (label, got, want, scale)


def test_coefficient_sets_are_what_they_claim():
    sets = {label: (rz0, a, b) for label, rz0, a, b in lv.coefficient_sets()}
    assert [len(sets[f"k{k}"][1]) for k in (1, 2, 3, 30, 343)] == [1, 2, 3, 30, 343]
    lam = np.linalg.eigvalsh(lv.tridiagonal(*sets["clustered"][1:]))
    assert lam.max() - lam.min() <= 2e-5 and abs(lam.mean() - 4.) <= 1e-5 and len(lam) == 20
    # k = 1: T = [1 / a_0], the value in closed form
    rz0, a, b = sets["k1"]
    st, got = entry(rz0, a, b)
    lg = math.log(1. / a[0])  # (the rounding of 1 / a_0 moves the logarithm by u, whatever its size)
    assert st == capi.AGP_OK and abs(got - rz0 * lg) <= 4 * 2. ** -53 * rz0 * (1. + abs(lg))


def test_statuses():
    # no iteration: the quadrature of nothing
    st, got = entry(2., np.zeros(0), np.zeros(0))
    assert st == capi.AGP_OK and got == 0.
    # T = [[1, 2], [2, 1]] has the eigenvalue -1: a_0 = 1, b_1 = 4, 1 / a_1 + b_1 / a_0 = 1
    st, got = entry(1., np.array([1., -1. / 3.]), np.array([0., 4.]))
    assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and got == -7.5
    st, got = entry(1., np.array([1., 1e30]), np.array([0., 4.]))  # 1 / a_1 + 4 = 4 + tiny: [[1, 2], [2, 4]] is singular
    assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and got == -7.5
    for a, b in (([1., float("nan")], [0., 1.]), ([1., 1.], [0., -1.]), ([0., 1.], [0., 1.]), ([1., 1.], [0., float("inf")])):
        st, got = entry(1., np.array(a), np.array(b))
        assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and got == -7.5, (a, b)
    st, got = entry(0., np.array([1.]), np.array([0.]))
    assert st == capi.AGP_ERR_NOT_POSITIVE_DEFINITE and got == -7.5


# ---- the restatement against the bars of the GPU file ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rank", lv.EXACT_SHAPES)
def test_exhausting_probes_are_exact_and_defects_are_not(name, rank):
    tc.identity_case(name)
    P = lv.preconditioner(name, rank)
    assert P.rank == rank
    A, _, _ = tc.dense_system(name)
    n = A.shape[0]
    Z = lv.exhausting_probes(P.L, P.delta)
    assert Z.shape == (n, n + rank)
    assert np.abs(Z @ Z.T / Z.shape[1] - (P.L @ P.L.T + P.delta * np.eye(n))).max() <= 1e-12 * P.d0
    ld, nll = lv.dense_values(name)
    got = lv.value_restated(name, rank, Z)
    print(f"{name} rank {rank}: log det {got['log_det']:.10g} against {ld:.10g} ({abs(got['log_det'] - ld):.3g}), "
          f"NLL {abs(got['nll'] - nll):.3g} off, bar {lv.parity_bar(n, ld):.3g}; iterations {got['iterations'].min()}..{got['iterations'].max()}")
    assert abs(got["log_det"] - ld) <= lv.parity_bar(n, ld)
    assert abs(got["nll"] - nll) <= lv.parity_bar(n, nll)
    # the entry on the same coefficients gives the same log-determinant
    s = np.zeros(Z.shape[1])
    for c in range(Z.shape[1]):
        rz0, a, b, _ = lv.pcg_coefficients(A, P, Z[:, c])
        st, s[c] = entry(rz0, a, b)
        assert st == capi.AGP_OK
    assert abs(lv.log_det_p(P) + s.sum() / len(s) - ld) <= lv.parity_bar(n, ld)
    # the samples are the exact u^T log(M) u
    exact = lv.exact_samples(name, P, Z)
    assert np.all(np.abs(got["samples"] - exact) <= lv.SAMPLE_BAR * got["scales"])
    for mut in lv.MUTATIONS:
        bad = lv.value_restated(name, rank, Z, mutation=mut)
        r = abs(bad["log_det"] - ld) / lv.parity_bar(n, ld)
        print(f"{name} rank {rank}: {mut}, error / bar {r:.3g}")
        assert not r <= 1e3, (mut, r)  # (a T that is no longer positive definite gives a NaN: a miss as well)


def test_seeded_estimate_is_within_two_standard_errors():
    name, rank, t, seed = lv.ESTIMATE
    P = lv.preconditioner(name, rank)
    Z = lv.seeded_probes(seed, P.L, P.delta, t)
    ld, nll = lv.dense_values(name)
    got = lv.value_restated(name, rank, Z)
    z = abs(got["log_det"] - ld) / got["log_det_stderr"]
    print(f"{name} rank {rank} t {t} seed {seed}: log det {got['log_det']:.6g} +- {got['log_det_stderr']:.3g}, dense {ld:.6g}: "
          f"{z:.2f} standard errors")
    assert z < 2., z
    assert got["log_det_stderr"] <= 0.01 * abs(ld)  # a loose stderr cannot carry the test above
    assert abs(got["nll"] - nll) < 2. * got["nll_stderr"]
    exact = lv.exact_samples(name, P, Z)
    assert np.all(np.abs(got["samples"] - exact) <= lv.SAMPLE_BAR * got["scales"])
    # the gradient from the same probes: E[w^T dA v] = tr(A^-1 dA)
    gs, _ = lv.gradient_samples_restated(name, P, Z)
    want, _ = tc.dense_gradient_nll(name)
    A, dA, alpha = tc.dense_system(name)
    for nm, smp in gs.items():
        g = 0.5 * smp.mean() - 0.5 * float(alpha @ dA[nm] @ alpha)
        gse = 0.5 * math.sqrt(((smp - smp.mean()) ** 2).sum() / (t * (t - 1)))
        print(f"{name} {nm}: {abs(g - want[nm]) / gse:.2f} standard errors from the dense gradient")
        assert abs(g - want[nm]) <= 4. * gse, nm


def test_probe_columns_depend_on_seed_and_column_alone():
    P = lv.preconditioner("n65_3d", 16)
    a, b = lv.seeded_probes(5, P.L, P.delta, 17), lv.seeded_probes(5, P.L, P.delta, 16)
    assert np.array_equal(a[:, :16], b) and not np.array_equal(a, lv.seeded_probes(6, P.L, P.delta, 17))
    g1, g2 = lv.normals(5, 65, 16, 4)
    assert not np.array_equal(g1, g2[:16])  # the factor's normals are a stream of their own
    want, bound = lv.probe_reference(P.L, P.delta, g1, g2)
    assert np.all(np.abs(lv.seeded_probes(5, P.L, P.delta, 4) - want) <= bound)
    assert math.isnan(lv.value_restated("n65_3d", 16, a[:, :1])["log_det_stderr"])
