"""CPU tests (no GPU) of agp_fit_update_batch's host side: the C-ABI declaration and its ctypes binding, and what
ab.update_batch rejects before it touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_batched_update():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    m = re.search(r"AGP_API int agp_fit_update_batch\((.*?)\);", text, re.S)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == [
        "agp_context *ctx", "int count",
        "const agp_kernel *const *kernels", "const agp_fit *const *olds",
        "const agp_features *const *x_new", "const double *y_new", "int64_t ldy",
        "const double *y_var_new", "int64_t ldv",
        "agp_fit **out", "double *information", "int64_t ldi",
        "double *log_det", "int *status",
    ]


def test_binding_matches_the_declaration():
    res, argt = {name: (res, argt) for name, res, argt in capi.EXPORTS}["agp_fit_update_batch"]
    assert res is C.c_int
    P, I64 = C.c_void_p, C.c_int64
    assert argt == [P, C.c_int, P, P, P, P, I64, P, I64, P, P, I64, P, P]
    assert hasattr(capi.load(), "agp_fit_update_batch")


class _NoDevice:
    """a context that must never be reached: every attribute access is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"update_batch touched the context ({name}) before rejecting its arguments")


def _fit_models(count, fit_type=abgp.GPFit):
    """FitModels over fits that hold no device handle (the checks under test come before any device call)"""
    dead = _NoDevice()
    out = []
    for b in range(count):
        model = ab.gp_from_covariance(ab.Matern52(2.0 + 0.1 * b, 1.0) + ab.IndependentNoise(0.1), context=dead)
        fit = fit_type.__new__(fit_type)  # no __init__: no handle to destroy
        fit.train_features = np.zeros((4, 3))
        out.append(abgp.FitModel(model, fit))
    return out


def _datasets(sizes):
    return [ab.RegressionDataset(np.zeros((m, 3)), np.zeros(m)) for m in sizes]


def test_rejects_an_empty_list():
    with pytest.raises(ValueError, match="at least one"):
        ab.update_batch([], [])


def test_rejects_unequal_lengths():
    with pytest.raises(ValueError, match="as many datasets as fit models"):
        ab.update_batch(_fit_models(3), _datasets([5, 5]))


def test_rejects_unequal_m():
    with pytest.raises(ValueError, match="same number of points"):
        ab.update_batch(_fit_models(3), _datasets([5, 5, 4]))


def test_rejects_a_fit_that_is_no_plain_gpfit():
    fms = _fit_models(2)
    fms[1] = abgp.FitModel(fms[1].get_model(), abgp.UpdatedGPFit.__new__(abgp.UpdatedGPFit))
    with pytest.raises(ValueError, match="plain fp64 GPFit"):
        ab.update_batch(fms, _datasets([5, 5]))
    mixed = _fit_models(2)
    mixed[0].get_fit().mixed_precision = True
    with pytest.raises(ValueError, match="plain fp64 GPFit"):
        ab.update_batch(mixed, _datasets([5, 5]))


def test_rejects_linear_combination_features():
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    with pytest.raises(ValueError, match="LinearCombination"):
        ab.update_batch(_fit_models(2), [ab.RegressionDataset(np.zeros((2, 3)), np.zeros(2)), ab.RegressionDataset(lc, np.zeros(2))])
