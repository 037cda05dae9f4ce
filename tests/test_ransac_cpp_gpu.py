"""GPU test of the C++ names of GP RANSAC (include/albatross_amd/albatross.hpp: model.ransac, DefaultGPRansacStrategy,
gp_ransac_strategy, RansacConfig, the return codes): builds examples/ransac_check.cpp with g++ against the C-ABI library
and runs it on the reference's toy case; the example exits non-zero on a mismatch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")


@pytest.mark.gpu
def test_ransac_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "ransac_check"])
    run = subprocess.run([os.path.join(EX, "ransac_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ransac_check ok" in run.stdout and "FAILED" not in run.stdout
    rows = dict(line.split(",", 1) for line in run.stdout.strip().splitlines() if "," in line)
    assert rows["return_code"] == "success" and rows["consensus_size"] == "8"
    members = rows["consensus"].split()
    assert len(members) == 8 and "3" not in members and "5" not in members
    assert rows["chi_squared_consensus_size"] == "10"
