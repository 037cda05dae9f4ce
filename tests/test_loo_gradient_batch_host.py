"""CPU tests (no GPU) of agp_loo_nll_gradient_batch's host side: the C-ABI declaration and its ctypes binding, and the
Python layer's refusal of LinearCombination features."""
import ctypes as C
import os

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp
from test_nll_gradient_batch_host import _declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_batched_leave_one_out_gradient():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    args = _declaration(text, "agp_loo_nll_gradient_batch")
    assert args == [
        "agp_context *ctx", "int count",
        "const agp_kernel *const *kernels", "const agp_features *const *features",
        "const double *y", "int64_t ldy",
        "const double *y_var", "int64_t ldv",
        "const int *n_slots",
        "const agp_gradient_slot *const *slots",
        "const double *const *tangents", "int64_t ldt",
        "double *loo_nll",
        "double *grad_loo_nll", "int64_t ldg",
        "double *mean_weights", "int64_t ldw",
        "int *status",
    ]


def test_binding_matches_the_declaration():
    res, argt = {name: (res, argt) for name, res, argt in capi.EXPORTS}["agp_loo_nll_gradient_batch"]
    assert res is C.c_int
    P, I64 = C.c_void_p, C.c_int64
    assert argt == [P, C.c_int, P, P, P, I64, P, I64, P, P, P, I64, P, P, I64, P, I64, P]
    assert hasattr(capi.load(), "agp_loo_nll_gradient_batch")


def test_linear_combination_features_are_refused():
    """by _gradient_problem under the entry's name and by every public surface, before a context is needed"""
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1))
    ds = ab.RegressionDataset(lc, np.zeros(2))
    with pytest.raises(NotImplementedError, match="agp_loo_nll_gradient_batch"):
        abgp._gradient_problem(model, ds, "agp_loo_nll_gradient_batch")
    with pytest.raises(NotImplementedError):
        model.leave_one_out_likelihoods(ds, [{}, {"sigma_independent_noise": 0.2}])
    with pytest.raises(NotImplementedError):
        model.leave_one_out_likelihood_gradients(ds, [{}, {"sigma_independent_noise": 0.2}])
    with pytest.raises(NotImplementedError):
        ab.leave_one_out_likelihood_gradient_batch([model, model], [ds, ds])
