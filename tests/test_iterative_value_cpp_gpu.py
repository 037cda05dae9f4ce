"""GPU test of the C++ names of the matrix-free log-likelihood value (include/albatross_amd/albatross.hpp:
IterativeLikelihoodOptions, IterativeFitModel::log_likelihood and ::log_likelihood_and_gradient): builds
examples/iterative_likelihood_check.cpp with g++ against the C-ABI library and runs it; the example compares value and
gradient from exhausting probes against the dense fit, checks the seeded estimate against the stated functions of its
samples, each difference relative to its bar, and exits non-zero on a mismatch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")


@pytest.mark.gpu
def test_iterative_likelihood_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "iterative_likelihood_check"])
    run = subprocess.run([os.path.join(EX, "iterative_likelihood_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = dict(line.split(",") for line in run.stdout.strip().splitlines() if "," in line)
    assert "iterative_likelihood_check ok" in run.stdout
    for name in ("exhausting_value_over_bar", "exhausting_gradient_over_bar", "seeded_functions_of_the_samples_over_bar",
                 "seeded_value_standard_errors_from_dense_over_4"):
        assert 0. <= float(rows[name]) <= 1., (name, rows[name])
    assert 0. <= float(rows["loose_quadrature_moved_the_value_by_standard_errors"]) <= 1e-3
    for name in ("mean_parameter_standard_error", "second_call_differs", "one_probe_standard_error_is_not_nan",
                 "loose_quadrature_is_not_shorter", "zero_fit_iterations", "one_iteration_did_not_raise"):
        assert float(rows[name]) == 0., (name, rows[name])
    assert int(rows["probe_iterations"]) > 0
