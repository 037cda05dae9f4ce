"""GPU test of the C++ surface of the ragged batch (include/albatross_amd/albatross.hpp: model.fit_batch,
albatross::predict_batch and albatross::update_batch over size classes): builds examples/ragged_batch_check.cpp with g++
against the C-ABI library and runs it; the example fits two models on seven datasets of unequal sizes each, predicts and
updates them in batches and prints the largest differences from the per-model fit / predict / update loop, which must
stay inside the bounds of tests/test_update_batch_cpp_gpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")


@pytest.mark.gpu
def test_ragged_batch_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "ragged_batch_check"])
    run = subprocess.run([os.path.join(EX, "ragged_batch_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ragged_batch_check ok" in run.stdout
    rows = {k: float(v) for k, v in (line.split(",") for line in run.stdout.strip().splitlines() if "," in line)}
    print(run.stdout)
    assert rows["problems"] == 14
    for name in ("information", "mean", "updated_information", "updated_mean"):
        assert rows[name + "_scale"] > 0.
        assert rows[name + "_diff"] <= 1e-8 * rows[name + "_scale"], name
    for name in ("marginal_variance", "joint_covariance", "updated_marginal_variance"):
        assert rows[name + "_scale"] > 0.
        assert rows[name + "_diff"] <= 1e-8 * rows[name + "_scale"] + 1e-9, name
