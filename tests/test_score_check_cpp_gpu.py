"""GPU test of the C++ names of the prediction scores (include/albatross_amd/albatross.hpp: albatross::score::energy_score,
variogram_score, crps_normal, albatross::ChiSquaredCdf): builds examples/score_check.cpp with g++ against the C-ABI
library and runs it; the example compares every name with values it computes through the C-ABI and exits non-zero on a
mismatch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")


@pytest.mark.gpu
def test_score_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "score_check"])
    run = subprocess.run([os.path.join(EX, "score_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = dict(line.split(",") for line in run.stdout.strip().splitlines() if "," in line)
    assert "score_check ok" in run.stdout
    for name in ("energy_score", "energy_score_marginal_weighted", "variogram_score", "variogram_score_marginal_weighted",
                 "chi_squared_cdf", "crps_centre"):
        assert name in rows
    assert float(rows["energy_score"]) > 0. and float(rows["variogram_score"]) > 0.
    assert 0. <= float(rows["chi_squared_cdf"]) <= 1.
