"""GPU test of the C++ surface of the batched leave-one-group-out gradient (include/albatross_amd/albatross.hpp:
model.leave_one_group_out_likelihood_gradient_batch over size classes, both predict types): builds
examples/logo_gradient_batch_check.cpp with g++ against the C-ABI library and runs it; the example evaluates one model on
seven datasets of unequal sizes, grouped by a callable, in batches and prints the largest differences from the per-dataset
loop over leave_one_group_out_likelihood_gradient.  Values agree to 1e-10 relative; the gradient of a parameter to 1e-9 of
its scale, the sum over the datasets of the magnitudes of the loop's gradients of that parameter - the bound of
test_ragged_gradient_batch_cpp_gpu.py, no wider than the 1e-9 s_p of the Python tests (s_p, the sum of the magnitudes of one
gradient's terms, is no smaller than that gradient's magnitude)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
PARAMETERS = ["elevation_scaling_center", "elevation_scaling_factor", "sigma_constant", "matern_52_length_scale", "sigma_matern_52",
              "sigma_independent_noise", "slope", "offset"]


@pytest.mark.gpu
def test_logo_gradient_batch_check_example():
    subprocess.check_call(["make", "-s", "-C", EX, "logo_gradient_batch_check"])
    run = subprocess.run([os.path.join(EX, "logo_gradient_batch_check")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "logo_gradient_batch_check ok" in run.stdout
    rows = {k: float(v) for k, v in (line.split(",") for line in run.stdout.strip().splitlines() if "," in line)}
    print(run.stdout)
    assert rows["problems"] == 7
    for metric in ("joint", "marginal"):
        assert rows[metric + "_value_rel"] <= 1e-10, metric
        names = sorted(k[len(metric) + len("_diff_"):] for k in rows if k.startswith(metric + "_diff_"))
        assert names == sorted(PARAMETERS)
        for name in names:
            scale = rows[f"{metric}_scale_{name}"]
            assert scale > 0., (metric, name)
            assert rows[f"{metric}_diff_{name}"] <= 1e-9 * scale, (metric, name)
