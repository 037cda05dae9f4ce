"""CPU tests (no GPU) of agp_predict_batch's host side: the C-ABI declaration and its ctypes binding, and what
ab.predict_batch rejects before it touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_batched_prediction():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    m = re.search(r"AGP_API int agp_predict_batch\((.*?)\);", text, re.S)
    assert m
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == [
        "agp_context *ctx", "int count",
        "const agp_kernel *const *kernels", "const agp_fit *const *fits",
        "const agp_features *const *xs", "int mode",
        "double *mean", "int64_t ldm",
        "double *second", "int64_t lds",
        "int out_location", "int *status",
    ]


def test_binding_matches_the_declaration():
    res, argt = {name: (res, argt) for name, res, argt in capi.EXPORTS}["agp_predict_batch"]
    assert res is C.c_int
    P, I64 = C.c_void_p, C.c_int64
    assert argt == [P, C.c_int, P, P, P, C.c_int, P, I64, P, I64, C.c_int, P]
    assert hasattr(capi.load(), "agp_predict_batch")


class _NoDevice:
    """a context that must never be reached: every attribute access is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"predict_batch touched the context ({name}) before rejecting its arguments")


def _fit_models(count, fit_type=abgp.GPFit):
    """FitModels over fits that hold no device handle (the checks under test come before any device call)"""
    dead = _NoDevice()
    out = []
    for b in range(count):
        model = ab.gp_from_covariance(ab.Matern52(2.0 + 0.1 * b, 1.0) + ab.IndependentNoise(0.1), context=dead)
        fit = fit_type.__new__(fit_type)  # no __init__: no handle to destroy
        out.append(abgp.FitModel(model, fit))
    return out


def test_rejects_unequal_m():
    fms = _fit_models(3)
    xs = [np.zeros((5, 3)), np.zeros((5, 3)), np.zeros((4, 3))]
    with pytest.raises(ValueError, match="same number of points"):
        ab.predict_batch(fms, xs)


def test_rejects_an_empty_list():
    with pytest.raises(ValueError, match="at least one"):
        ab.predict_batch([], np.zeros((5, 3)))


def test_rejects_an_unknown_what():
    with pytest.raises(ValueError, match="what"):
        ab.predict_batch(_fit_models(2), np.zeros((5, 3)), what="variance")


def test_rejects_a_fit_that_is_no_plain_gpfit():
    fms = _fit_models(2)
    fms[1] = abgp.FitModel(fms[1].get_model(), abgp.UpdatedGPFit.__new__(abgp.UpdatedGPFit))
    with pytest.raises(ValueError, match="plain fp64 GPFit"):
        ab.predict_batch(fms, np.zeros((5, 3)))
    mixed = _fit_models(2)
    mixed[0].get_fit().mixed_precision = True
    with pytest.raises(ValueError, match="plain fp64 GPFit"):
        ab.predict_batch(mixed, np.zeros((5, 3)))


def test_rejects_linear_combination_features_and_a_wrong_number_of_feature_vectors():
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    with pytest.raises(ValueError, match="LinearCombination"):
        ab.predict_batch(_fit_models(2), lc)
    with pytest.raises(ValueError, match="LinearCombination"):
        ab.predict_batch(_fit_models(2), [np.zeros((2, 3)), lc])
    with pytest.raises(ValueError, match="one feature vector per fit model"):
        ab.predict_batch(_fit_models(3), [np.zeros((2, 3)), np.zeros((2, 3))])
