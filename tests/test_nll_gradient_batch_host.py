"""CPU tests (no GPU) of agp_nll_gradient_batch's host side: the C-ABI declaration and its ctypes binding, and the
per-problem slot tables and tangent columns the Python layer assembles for a batch of parameter overrides."""
import ctypes as C
import os
import re

import numpy as np

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Elevation(ab.ScalingFunction):
    _params = {"elevation_scaling_center": 4.0, "elevation_scaling_factor": 0.3}

    def _call_impl(self, c):
        p = self.get_params()
        return 1. + p["elevation_scaling_factor"] * np.maximum(p["elevation_scaling_center"] - np.asarray(c)[:, 2], 0.)


def _declaration(text, name):
    m = re.search(r"AGP_API int " + name + r"\((.*?)\);", text, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_batched_gradient():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    args = _declaration(text, "agp_nll_gradient_batch")
    assert args == [
        "agp_context *ctx", "int count",
        "const agp_kernel *const *kernels", "const agp_features *const *features",
        "const double *y", "int64_t ldy",
        "const double *y_var", "int64_t ldv",
        "const int *n_slots",
        "const agp_gradient_slot *const *slots",
        "const double *const *tangents", "int64_t ldt",
        "double *nll",
        "double *grad_nll", "int64_t ldg",
        "double *information", "int64_t ldi",
        "int *status",
    ]


def test_binding_matches_the_declaration():
    entry = {name: (res, argt) for name, res, argt in capi.EXPORTS}["agp_nll_gradient_batch"]
    res, argt = entry
    assert res is C.c_int
    P, I64 = C.c_void_p, C.c_int64
    assert argt == [P, C.c_int, P, P, P, I64, P, I64, P, P, P, I64, P, P, I64, P, I64, P]
    assert hasattr(capi.load(), "agp_nll_gradient_batch")


def test_slot_assembly_per_override():
    """the helper gives every problem of a batch the slot table of its own copy, and ScalingTerm tangent columns taken
    at that copy's parameters"""
    rng = np.random.default_rng(3)
    x = rng.uniform(0., 10., (40, 3))
    y = np.sin(x).sum(axis=1)
    cov = ab.ScalingTerm(_Elevation()) * ab.Constant(0.5) + ab.Matern52(2.0, 1.0) + ab.IndependentNoise(0.1)
    model = ab.gp_from_covariance_and_mean(cov, ab.LinearMean(0.2, -0.4))
    ds = ab.RegressionDataset(x, y)
    sets = [{}, {"elevation_scaling_center": 6.0}, {"elevation_scaling_factor": 0.9, "sigma_matern_52": 1.5}, {"slope": 1.0}]
    copies = model._override_copies(sets)
    assert len(copies) == len(sets)
    for m, overrides in zip(copies, sets):
        p = abgp._gradient_problem(m, ds)
        slots, columns = m.covariance_function_.param_slots()
        assert p.slots == slots
        assert [(t.node, t.param) for t in p.table][:len(slots)] == [(node, param) for node, param, _ in slots]
        assert p.tangents is not None and p.tangents.shape == (40, len(columns)) and p.tangents.flags.f_contiguous
        center = overrides.get("elevation_scaling_center", 4.0)
        factor = overrides.get("elevation_scaling_factor", 0.3)
        for c, (fn, name) in enumerate(columns):
            # d f / d name at the copy's own parameters
            if name == "elevation_scaling_factor":
                want = np.maximum(center - x[:, 2], 0.)
            else:
                want = factor * (center - x[:, 2] > 0.)
            np.testing.assert_allclose(p.tangents[:, c], want, rtol=1e-6, atol=1e-8)
        # targets with the copy's own mean removed
        slope = overrides.get("slope", 0.2)
        mean = m.mean_function_(x)
        np.testing.assert_allclose(p.y, y - mean)
        assert m.get_params()["slope"] == slope
    # the copies are independent of the model and of each other
    assert model.get_params()["elevation_scaling_center"] == 4.0
    assert copies[1].get_params()["elevation_scaling_center"] == 6.0


def test_slot_assembly_without_scaling_terms():
    x = np.linspace(0., 1., 10)
    cov = ab.Polynomial(2, 0.8) + ab.IndependentNoise(0.1)
    p = abgp._gradient_problem(ab.gp_from_covariance(cov), ab.RegressionDataset(x, x))
    assert p.tangents is None
    assert len(p.slots) == 4 and p.slots == cov.param_slots()[0]


def test_linear_combination_features_are_refused():
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    model = ab.gp_from_covariance(ab.SquaredExponential(1.0, 1.0) + ab.IndependentNoise(0.1))
    try:
        abgp._gradient_problem(model, ab.RegressionDataset(lc, np.zeros(2)), "agp_nll_gradient_batch")
    except NotImplementedError:
        pass
    else:
        raise AssertionError("LinearCombination features must raise")
