"""GPU test of the C++ surface of the batched update (include/albatross_amd/albatross.hpp: albatross::update_batch over
agp_fit_update_batch): builds examples/update_batch_check.cpp with g++ against the C-ABI library and runs it; the example
updates the FitModels of two fit_batch calls in one call and prints the largest difference of the information vectors
and the predictions of the grown fits from the per-model update() loop, which must stay inside the bounds of
tests/test_predict_batch_cpp_gpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")


@pytest.mark.gpu
def test_update_batch_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "update_batch_check"])
    run = subprocess.run([os.path.join(EX, "update_batch_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "update_batch_check ok" in run.stdout
    rows = {k: float(v) for k, v in (line.split(",") for line in run.stdout.strip().splitlines() if "," in line)}
    print(run.stdout)
    assert rows["problems"] == 6
    for name in ("information", "mean"):
        assert rows[name + "_scale"] > 0.
        assert rows[name + "_diff"] <= 1e-8 * rows[name + "_scale"], name
    for name in ("marginal_variance", "joint_covariance"):
        assert rows[name + "_scale"] > 0.
        assert rows[name + "_diff"] <= 1e-8 * rows[name + "_scale"] + 1e-9, name
