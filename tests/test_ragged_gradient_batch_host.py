"""CPU tests (no GPU) of the host side of the ragged batched gradients: the C-ABI declarations of
agp_nll_gradient_batch_ragged and agp_loo_nll_gradient_batch_ragged and their ctypes bindings (the argument lists of the
equal-size entries, exactly), the exported symbols, the Python and C++ surfaces, and what the Python batch functions reject
before they touch the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from test_nll_gradient_batch_host import _declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [("agp_nll_gradient_batch_ragged", "agp_nll_gradient_batch"), ("agp_loo_nll_gradient_batch_ragged", "agp_loo_nll_gradient_batch")]


def test_header_declares_both_entries_with_the_arguments_of_their_twins():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    for ragged, twin in PAIRS:
        args = _declaration(text, ragged)
        assert len(args) == 18 and args[0] == "agp_context *ctx" and args[-1] == "int *status"
        assert args == _declaration(text, twin), ragged
    assert _declaration(text, "agp_nll_gradient_batch_ragged")[12:17] == [
        "double *nll", "double *grad_nll", "int64_t ldg", "double *information", "int64_t ldi"]
    assert _declaration(text, "agp_loo_nll_gradient_batch_ragged")[12:17] == [
        "double *loo_nll", "double *grad_loo_nll", "int64_t ldg", "double *mean_weights", "int64_t ldw"]


def test_bindings_have_the_types_of_the_twins():
    table = {name: (res, argt) for name, res, argt in capi.EXPORTS}
    P, I64 = C.c_void_p, C.c_int64
    for ragged, twin in PAIRS:
        assert table[ragged] == (C.c_int, [P, C.c_int, P, P, P, I64, P, I64, P, P, P, I64, P, P, I64, P, I64, P])
        assert table[ragged] == table[twin]


def test_library_exports_both_symbols():
    lib = capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path()], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for ragged, _ in PAIRS:
        assert hasattr(lib, ragged)
        assert ragged in exported


def test_export_map_lists_them():
    """the linker script exports the agp_ prefix and nothing else: the new names are covered by it"""
    text = open(os.path.join(ROOT, "albatross_amd", "csrc", "exports.map")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    patterns = re.search(r"global:(.*?);", text, re.S).group(1).split()
    import fnmatch
    for ragged, _ in PAIRS:
        assert any(fnmatch.fnmatchcase(ragged, p) for p in patterns), ragged


def test_python_and_cpp_surfaces_exist():
    for name in ("pooled_log_likelihood_gradient", "pooled_leave_one_out_likelihood_gradient", "log_likelihood_gradient_batch",
                 "leave_one_out_likelihood_gradient_batch"):
        assert callable(getattr(ab, name)) and name in ab.__all__
    for fn in (ab.log_likelihood_gradient_batch, ab.leave_one_out_likelihood_gradient_batch):
        assert "of one size" not in fn.__doc__ and "same number of points" not in fn.__doc__
    hpp = open(os.path.join(ROOT, "include", "albatross_amd", "albatross.hpp")).read()
    assert re.search(r"std::vector<LogLikelihoodGradient>\s+log_likelihood_gradient_batch\(\s*const std::vector<RegressionDataset<FeatureType>> &", hpp)
    assert re.search(r"std::vector<LeaveOneOutLikelihoodGradient>\s+leave_one_out_likelihood_gradient_batch\(\s*const std::vector<RegressionDataset<FeatureType>> &", hpp)
    assert "agp_nll_gradient_batch_ragged" in hpp and "agp_loo_nll_gradient_batch_ragged" in hpp
    assert os.path.exists(os.path.join(ROOT, "examples", "ragged_gradient_check.cpp"))
    assert "ragged_gradient_check" in open(os.path.join(ROOT, "examples", "Makefile")).read()


class _NoDevice:
    """a context that must never be reached: every attribute access is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the batch touched the context ({name}) before rejecting its arguments")


def _models(contexts):
    return [ab.gp_from_covariance(ab.Matern52(2.0 + 0.1 * b, 1.0) + ab.IndependentNoise(0.1), context=c) for b, c in enumerate(contexts)]


def _dataset(n):
    return ab.RegressionDataset(np.zeros((n, 3)), np.zeros(n))


BATCHES = [ab.log_likelihood_gradient_batch, ab.leave_one_out_likelihood_gradient_batch]


@pytest.mark.parametrize("batch", BATCHES)
def test_batches_reject_unequal_list_lengths(batch):
    dead = _NoDevice()
    with pytest.raises(ValueError, match="as many datasets as models"):
        batch(_models([dead] * 3), [_dataset(5), _dataset(7)])
    with pytest.raises(ValueError, match="at least one"):
        batch([], [])


@pytest.mark.parametrize("batch", BATCHES)
def test_batches_reject_mixed_contexts(batch):
    """datasets of unequal sizes on models of two contexts: refused before any device call"""
    with pytest.raises(ValueError, match="one context"):
        batch(_models([_NoDevice(), _NoDevice(), _NoDevice()]), [_dataset(5), _dataset(7), _dataset(200)])


@pytest.mark.parametrize("pooled", [ab.pooled_log_likelihood_gradient, ab.pooled_leave_one_out_likelihood_gradient])
def test_pooled_helpers_reject_an_empty_list(pooled):
    with pytest.raises(ValueError, match="at least one"):
        pooled(_models([_NoDevice()])[0], [])
