"""GPU test of the C++ names of the matrix-free gradient (include/albatross_amd/albatross.hpp: albatross::gram_tangent_forms,
IterativeGradientOptions, IterativeFitModel::log_likelihood_gradient): builds examples/iterative_gradient_check.cpp with g++
against the C-ABI library and runs it; the example compares the probe gradient with identity probes against the dense fit's
exact gradient, checks the seeded estimate against the stated functions of its samples and the forms against central
differences, each difference relative to its bar, and exits non-zero on a mismatch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")


@pytest.mark.gpu
def test_iterative_gradient_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "iterative_gradient_check"])
    run = subprocess.run([os.path.join(EX, "iterative_gradient_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = dict(line.split(",") for line in run.stdout.strip().splitlines() if "," in line)
    assert "iterative_gradient_check ok" in run.stdout
    for name in ("identity_gradient_over_bar", "seeded_functions_of_the_samples_over_bar", "forms_against_central_differences_over_bar"):
        assert 0. <= float(rows[name]) <= 1., (name, rows[name])
    for name in ("mean_parameter_standard_error", "second_call_differs", "one_probe_standard_error_is_not_nan", "zero_fit_iterations",
                 "one_iteration_did_not_raise"):
        assert float(rows[name]) == 0., (name, rows[name])
    assert int(rows["probe_iterations"]) > 0
