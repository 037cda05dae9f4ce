"""The bounds of tests/gram_tangent_cases.py without a GPU: the plan the cases read agrees with its Python restatement, a
float64 numpy restatement of gram_tangent_kernel in the kernel's order meets every bound of the forms on the inputs the GPU
file uses, and four planted defects miss it by a large factor - a dropped column tile, the off-diagonal pair applied one way
only, the diagonal applied twice, column c of V read as c + 1.  The probe gradient's definition is restated the same way:
identity probes give the dense gradient, and the seeded estimate lies within four of its own standard errors of it."""
import math

import numpy as np
import pytest

import gram_tangent_cases as tc

pytestmark = pytest.mark.skipif(not tc.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no reference")


def test_plan_probe_agrees_with_its_restatement():
    for n in list(range(1, 1100)) + [4096, 16384, 65536, 262144, 262145]:
        p, r = tc.plan(n), tc.plan_restated(n)
        assert all(p[k] == r[k] for k in r), (n, p, r)
        assert p["rows"] == 256 and p["cols"] == 64 and p["group"] == 4 and p["max_pairs"] == 8
        assert p["units"] * p["slices"] <= 2 * tc.TARGET_WGS or p["slices"] == 1, (n, p)
    assert [tc.plan(1, c)["first_chunk"] for c in (1, 2, 4, 5, 8, 33)] == [1, 4, 4, 8, 8, 8]
    # scratch: one block of max_pairs x group doubles per workgroup, whatever n
    p = tc.plan(262144)
    assert p["units"] * p["slices"] * p["max_pairs"] * p["group"] * 8 < 1 << 20


def test_edge_sizes_cover_the_row_block_unit_and_slice_edges():
    e = tc.edge_sizes()
    cols, rows = tc.plan(1)["cols"], tc.plan(1)["rows"]
    for edge in list(range(cols, tc.N_MAX, cols)) + list(range(rows, tc.N_MAX, rows)):  # every column-tile and row-block edge
        for n in (edge - 1, edge, edge + 1):
            assert n in e, (n, e)
    slice_edges = [n for n in range(2, tc.N_MAX + 1) if tc.plan(n)["slices"] != tc.plan(n - 1)["slices"]]
    assert slice_edges and all(m in e for n in slice_edges for m in (n - 2, n - 1, n)), slice_edges
    assert len({tc.plan(n)["slices"] for n in e}) >= 3
    sizes = {s["n"] for s in tc.form_specs()}
    assert set(tc.N_BASE) <= sizes and set(e) <= sizes and max(sizes) <= tc.N_MAX
    specs = tc.form_specs()
    assert {s["ncols"] for s in specs} >= set(tc.NCOLS)
    assert {s.get("n_slots") for s in specs} >= set(tc.N_SLOTS)
    assert {s.get("dim", 3) for s in specs} >= set(tc.DIMS)


@pytest.mark.parametrize("spec", tc.HOST_SPECS, ids=[tc.spec_id(s) for s in tc.HOST_SPECS])
def test_kernel_order_restatement_meets_the_bound_and_defects_do_not(spec):
    case = tc.form_case(**spec)
    ref, scale, gamma = tc.reference(case)
    assert np.all(np.isfinite(scale)) and np.all(scale >= 0) and np.any(scale > 0)  # (a gated slot: exactly 0, form and scale)
    r = tc.ratio(tc.kernel_order_forms(case), case)
    print(f"{case.name}: plain float64 in kernel order, error / bound {r:.3g} (gamma {gamma / tc.U:.0f} U)")
    assert r <= 1., (case.name, r)
    if case.n < 65 or case.ncols < 2:
        return
    for mut in ("drop_tile", "one_way", "diag_twice", "next_column"):
        bad = tc.ratio(tc.kernel_order_forms(case, mut=(mut,)), case)
        print(f"{case.name}: {mut}, error / bound {bad:.3g}")
        assert bad > 1e3, (case.name, mut, bad)


# ---- the probe gradient, restated --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n65_3d", "n130_3d"])
def test_identity_probes_give_the_dense_gradient(name):
    cond = tc.identity_case(name)
    A, _, _ = tc.dense_system(name)
    n = A.shape[0]
    grad, _, _, _ = tc.gradient_restated(name, math.sqrt(n) * np.eye(n))
    want, scale = tc.dense_gradient_nll(name)
    worst = max(abs(grad[k] - want[k]) / scale[k] for k in want)
    print(f"{name}: cond(A) {cond:.3g}, identity probes against the dense gradient {worst:.3g} s_p")
    assert worst <= 1e-10, (name, worst)


def test_seeded_estimate_is_within_four_standard_errors():
    name, t, seed = "n777_2d", 64, 1
    A, _, _ = tc.dense_system(name)
    Z = tc.rademacher(seed, A.shape[0], t)
    assert set(np.unique(Z)) == {-1., 1.} and abs(Z.mean()) < 0.05
    grad, stderr, samples, _ = tc.gradient_restated(name, Z)
    want, _ = tc.dense_gradient_nll(name)
    for k in want:
        z = abs(grad[k] - want[k]) / stderr[k]
        rel = stderr[k] / (0.5 * abs(samples[k].mean()))
        print(f"{name} {k}: {z:.2f} standard errors from the dense gradient, relative standard error of the trace {rel:.3g}")
        assert z <= 4., (k, z)
        assert rel <= 0.05, (k, rel)  # a loose stderr cannot carry the test above


def test_probe_columns_depend_on_seed_and_column_alone():
    a, b = tc.rademacher(5, 65, 17), tc.rademacher(5, 65, 16)
    assert np.array_equal(a[:, :16], b) and not np.array_equal(a, tc.rademacher(6, 65, 17))
    _, se1, _, _ = tc.gradient_restated("n65_3d", a[:, :1])
    assert all(math.isnan(v) for v in se1.values())
