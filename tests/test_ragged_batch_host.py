"""CPU tests (no GPU) of the ragged batch's host side: the C-ABI declarations and their ctypes bindings, the size-class
rule, and what ab.fit_batch rejects before it touches the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
from albatross_amd import gp as abgp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name, result):
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    m = re.search(r"AGP_API %s %s\((.*?)\);" % (result, name), text, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_ragged_entries():
    ragged = _declared("agp_fit_create_batch_ragged", "int")
    assert ragged == [
        "agp_context *ctx", "int count", "const agp_kernel *const *kernels", "const agp_features *const *features",
        "const double *y", "int64_t ldy", "const double *y_var", "int64_t ldv", "agp_fit **out", "double *information",
        "int64_t ldi", "double *log_det", "int *status",
    ]
    assert ragged == _declared("agp_fit_create_batch", "int")  # the signature of the equal-size entry
    assert _declared("agp_fit_padded_size", "int64_t") == ["const agp_fit *fit"]


def test_bindings_match_the_declarations():
    table = {name: (res, argt) for name, res, argt in capi.EXPORTS}
    P, I64 = C.c_void_p, C.c_int64
    assert table["agp_fit_create_batch_ragged"] == (C.c_int, [P, C.c_int, P, P, P, I64, P, I64, P, P, I64, P, P])
    assert table["agp_fit_create_batch_ragged"] == table["agp_fit_create_batch"]
    assert table["agp_fit_padded_size"] == (I64, [P])
    lib = capi.load()
    assert hasattr(lib, "agp_fit_create_batch_ragged") and hasattr(lib, "agp_fit_padded_size")


def test_size_classes():
    assert abgp._size_classes([60, 128, 129, 250, 256, 300, 700]) == [[0, 1], [2, 3, 4], [5], [6]]
    assert abgp._size_classes([300, 300, 300]) == [[0, 1, 2]]  # equal sizes: one class, nothing padded
    assert abgp._size_classes([17]) == [[0]]
    # ascending classes whatever the caller's order, the caller's order inside a class
    assert abgp._size_classes([700, 1, 129, 128, 256]) == [[1, 3], [2, 4], [0]]
    sizes = list(np.random.default_rng(0).integers(1, 2000, 200))
    classes = abgp._size_classes(sizes)
    assert sorted(b for c in classes for b in c) == list(range(200))
    for members in classes:  # padding waste under 128 rows per problem
        assert max(sizes[b] for b in members) - min(sizes[b] for b in members) < 128


def test_padded_groups_keep_the_handles_of_one_call_neighbours():
    """groups by padded size in ascending order; inside a group the handles of one batched call in slot order, then the
    fits of calls of their own in the caller's order"""
    from types import SimpleNamespace as NS
    padded = {1: 256, 2: 128, 3: 256, 4: 256, 5: 128, 6: 256, 7: 256}
    ctx = NS(_lib=NS(agp_fit_padded_size=lambda h: padded[h]))
    origins = {1: (9, 1), 2: None, 3: (4, 0), 4: None, 5: (3, 0), 6: (9, 0), 7: (4, 1)}
    fms = []
    for h in range(1, 8):
        fit = NS(_h=h)
        if origins[h] is not None:
            fit._batch_origin = origins[h]
        fms.append(NS(_fit=fit))
    # positions:  0: 256 (9, 1)   1: 128 own   2: 256 (4, 0)   3: 256 own   4: 128 (3, 0)   5: 256 (9, 0)   6: 256 (4, 1)
    assert abgp._padded_groups(ctx, fms) == [[4, 1], [2, 6, 5, 0, 3]]


class _NoDevice:
    """a context that must never be reached: every attribute access is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"fit_batch touched the context ({name}) before rejecting its arguments")


def _models(count):
    dead = _NoDevice()
    return [ab.gp_from_covariance(ab.Matern52(2.0 + 0.1 * b, 1.0) + ab.IndependentNoise(0.1), context=dead) for b in range(count)]


def _dataset(n):
    return ab.RegressionDataset(np.zeros((n, 3)), np.zeros(n))


def test_fit_batch_rejects_unequal_list_lengths():
    with pytest.raises(ValueError, match="as many datasets as models"):
        ab.fit_batch(_models(3), [_dataset(5), _dataset(7)])
    with pytest.raises(ValueError, match="at least one"):
        ab.fit_batch([], [])


def test_fit_batch_rejects_a_model_that_is_not_fp64():
    models = _models(2)
    models[1].precision = "mixed"
    with pytest.raises(ValueError, match="fp64 models"):
        ab.fit_batch(models, [_dataset(5), _dataset(7)])


def test_fit_batch_rejects_linear_combination_features():
    lc = [ab.LinearCombination([0.1, 0.2], [0.5, 0.5]), ab.LinearCombination([0.7], [1.0])]
    with pytest.raises(ValueError, match="plain features"):
        ab.fit_batch(_models(2), [_dataset(5), ab.RegressionDataset(lc, np.zeros(2))])
