"""The bounds of tests/qr_cases.py can be met, and its inputs are what they are meant to be: on every case that
tests/test_qr_gpu.py gives to the kernels of csrc/qr.hip the pivots are unambiguous, the rank is clear of its
threshold, and the plain float64 restatement of the algorithm meets each bound with the slack the module's docstring
states.  So a correct kernel can pass those tests.  No GPU."""
import numpy as np
import pytest

import qr_cases as qc

CASES = qc.qr_cases()
NAMES = sorted({c["name"] for c in CASES}, key=[c["name"] for c in CASES].index)


@pytest.mark.parametrize("name", NAMES)
def test_inputs_meet_their_conditions(name):
    A, _, det = qc.qr_input(name)
    rows, cols = A.shape
    ref, f64 = qc.restated(name, "ref"), qc.restated(name, "f64")
    ok, gap = qc.pivot_gap_ok(name)
    margin = min(ref["rank_margin"], f64["rank_margin"])
    print(f"{name}: smallest pivot gap {gap:.3g}, rank margin {margin:.3g}, nonzero_pivots margin "
          f"{min(ref['np_margin'], f64['np_margin']):.3g}")
    assert ok, gap
    assert np.array_equal(ref["perm"][:det], f64["perm"][:det])
    assert sorted(f64["perm"]) == list(range(cols))
    assert margin >= qc.RANK_MARGIN, margin
    assert ref["rank"] == f64["rank"]
    assert qc.counts_determined(name) == (name not in qc.NP_EXEMPT)
    if name in qc.SPECIAL:
        return
    assert ref["nonzero_pivots"] == cols and ref["rank"] == cols


def test_special_inputs_are_what_they_are_for():
    z = qc.restated("zeros", "ref")
    assert z["nonzero_pivots"] == 20 and z["rank"] == 20
    assert np.all(z["tau"][20:] == 0) and np.all(z["qr"][20:, 20:50] == 0)
    # no swap once every remaining norm is zero: the first index wins each tie
    assert np.array_equal(z["perm"], qc.after_swaps(z["perm"], 20))
    c = qc.restated("zerocol", "ref")
    assert c["perm"][11] == 5 and c["nonzero_pivots"] == 11 and c["rank"] == 11 and c["tau"][11] == 0
    A, _, _ = qc.qr_input("tie")
    assert np.array_equal(A[:, 2], A[:, 40]) and np.argmax((A * A).sum(axis=0)) == 2
    t = qc.restated("tie", "ref")
    assert t["perm"][0] == 2 and t["gap"][0] == 0.0 and t["rank"] == 69
    assert qc.restated("lowrank", "ref")["rank"] == qc.LOWRANK[1] == qc.restated("lowrank", "f64")["rank"]


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restated_qr_meets_bounds(case):
    name, extra = case["name"], case["extra"]
    cols = qc.qr_input(name)[0].shape[1]
    f = qc.restated(name, "f64")
    qr = f["qr"][:, :cols + extra]
    t = qc.tau_ratio(qr, f["tau"], cols)
    b = qc.backward_ratio(name, extra, qr, f["tau"], f["perm"])
    fw, below = qc.forward_ratios(name, extra, qr, f["perm"])
    print(f"{case['id']}: tau {t:.3g}, backward {b:.3g}, forward {fw:.3g}, below the rank {below:.3g}")
    assert t <= 1.0 and b <= 1.0
    assert qc.helper_ratio(name, f["threshold_helper"]) <= 1.0
    assert fw <= qc.RESTATEMENT_SLACK and below <= qc.RESTATEMENT_SLACK


@pytest.mark.parametrize("m,nrhs", qc.SQRT_SHAPES)
def test_restated_sqrt_solve_meets_bound(m, nrhs):
    R, perm = qc.square_factor(m)
    X = qc.solve_rhs(m, nrhs)
    ratio = qc.sqrt_solve_ratio(R, perm, X, qc.sqrt_solve(R, perm, X))
    print(f"sqrt_solve m={m} nrhs={nrhs}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("m,npv", qc.BACK_SHAPES)
def test_restated_back_solve_meets_bound(m, npv):
    R, perm = qc.square_factor(m)
    c = qc.solve_rhs(m, 1)[:, 0]
    out, z = qc.back_solve(R, perm, npv, c)
    ratio = qc.back_solve_ratio(R, npv, c, z)
    print(f"back_solve m={m} np={npv}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio
    assert np.all(out[perm[npv:]] == 0.0) and np.array_equal(out[perm[:npv]], z)


def test_bounds_are_not_slack_for_a_wrong_factor():
    """The checks refuse what the GPU tests are there to catch: one element of R off in the tenth digit, one row of a
    reflector not scaled, one element of a trailing column not updated, a solve that stops one row early."""
    name = "300x129"
    cols = 129
    f = qc.restated(name, "f64")
    qr, tau, perm = f["qr"], f["tau"], f["perm"]
    assert qc.backward_ratio(name, 1, qr, tau, perm) <= 1.0
    bad = qr.copy()
    bad[100, 120] *= 1.0 + 1e-10
    assert qc.forward_ratios(name, 1, bad, perm)[0] > 1.0
    bad[100, 120] *= 1.0 + 1e-7  # (c steps rows u = 1.7e-11 of the column's NORM, which this element is a small part of)
    assert qc.backward_ratio(name, 1, bad, tau, perm) > 1.0
    bad = qr.copy()
    bad[299, 3] *= 1.0 + 1e-6   # the last row of a reflector: the ragged tail of a 256-wide trip
    assert qc.tau_ratio(bad, tau, cols) > 1.0 or qc.backward_ratio(name, 1, bad, tau, perm) > 1.0
    bad = qr.copy()
    bad[128, cols] += 1e-10     # Q^T y
    assert qc.forward_ratios(name, 1, bad, perm)[0] > 1.0
    R, p = qc.square_factor(129)
    X = qc.solve_rhs(129, 5)
    W = qc.sqrt_solve(R, p, X)
    W[128, 4] *= 1.0 + 1e-9
    assert qc.sqrt_solve_ratio(R, p, X, W) > 1.0
    c = qc.solve_rhs(129, 1)[:, 0]
    _, z = qc.back_solve(R, p, 64, c)
    z[0] *= 1.0 + 1e-9
    assert qc.back_solve_ratio(R, 64, c, z) > 1.0
