"""The tangent bilinear forms on the device, through the public entry: agp_gram_tangent_forms (csrc/gram_tangent.hip) and
ab.gram_tangent_forms.

Cases, reference, scale and bound are tests/gram_tangent_cases.py's (its docstring derives the bound;
tests/test_gram_tangent_host.py shows that plain float64 in the kernel's order stays far inside it and that four kinds of
defect do not).  Every case asserts error / bound <= 1 against the longdouble reference and prints the ratio.  U, V and the
tangent columns sit in NaN buffers with ld > n and a NaN column behind them; forms goes in full of canaries and keeps their
bits outside its ncols x n_slots block; both locations run and give the same bits; two calls give the same bits."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import contraction_cases as cc
import gram_path_cases as gp
import gram_tangent_cases as tc

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not tc.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no reference")]

WORST = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


SPECS = tc.form_specs()


@pytest.mark.parametrize("spec", SPECS, ids=[tc.spec_id(s) for s in SPECS])
def test_forms_meet_the_bound(ctx, spec):
    case = tc.form_case(**spec)
    P = len(case.slots)
    st, forms, buf, ldf = tc.run_forms(ctx, case, capi.HOST)
    assert st == capi.AGP_OK, st
    r = tc.ratio(forms, case)
    WORST["forms"] = max(WORST.get("forms", 0.), r)
    print(f"{case.name}: error / bound {r:.3g} (worst so far {WORST['forms']:.3g}), plan {tc.plan(case.n)}")
    assert r <= 1., (case.name, r)
    assert tc.untouched(buf, ldf, case.ncols, P)
    st2, forms2, buf2, _ = tc.run_forms(ctx, case, capi.HOST)
    assert st2 == capi.AGP_OK and same_bits(buf, buf2)
    st3, forms3, buf3, _ = tc.run_forms(ctx, case, capi.DEVICE)
    assert st3 == capi.AGP_OK and same_bits(buf, buf3)


def test_python_surface_sums_slots_by_name(ctx):
    case = tc.form_case("scaling", 129, 5)
    _, forms, _, _ = tc.run_forms(ctx, case)
    x = case.fs.coords
    got = ab.gram_tangent_forms(case.cov, ab.Measurement(x), case.U, case.V, context=ctx)
    names = [nm for _, _, nm in case.cov.param_slots()[0]]
    assert set(got) == set(names)
    _, scale, _ = tc.reference(case)
    scaling = {nm for (node, _), nm in zip(case.slots, names) if case.nodes[node]["op"] == capi.OP_SCALING}
    assert scaling and scaling != set(names)
    for nm in set(names):
        mine = [p for p, q in enumerate(names) if q == nm]
        want = sum(forms[:, p] for p in mine)
        if nm in scaling:  # the Python surface takes a central difference of the scaling function, the case its analytic tangent
            assert np.all(np.abs(got[nm] - want) <= 1e-6 * sum(scale[:, p] for p in mine)), nm
        else:
            assert same_bits(got[nm], want), nm
    one = ab.gram_tangent_forms(case.cov, ab.Measurement(x), case.U[:, 0], case.V[:, 0], names=[names[0]], context=ctx)
    assert list(one) == [names[0]] and one[names[0]].shape == (1,)
    # the bytes of a column-major n x ncols matrix on the device
    Ud, Vd = (ctx.to_device(np.ascontiguousarray(M.T)) for M in (case.U, case.V))
    Ud.shape = Vd.shape = case.U.shape
    dev = ab.gram_tangent_forms(case.cov, ab.Measurement(x), Ud, Vd, on_device=True, context=ctx)
    for nm in got:
        assert same_bits(dev[nm], got[nm]), nm
    with pytest.raises(KeyError):
        ab.gram_tangent_forms(case.cov, x, case.U, case.V, names=["no_such_parameter"], context=ctx)


def test_the_shared_name_of_two_leaves(ctx):
    cov = ab.SquaredExponential(1.0, 1.0) + ab.SquaredExponential(1.0, 1.0) * ab.Constant(0.5) + ab.IndependentNoise(0.1)
    rng = np.random.default_rng(3)
    x, Um, Vm = rng.uniform(0., 4., (65, 3)), rng.standard_normal((65, 2)), rng.standard_normal((65, 2))
    got = ab.gram_tangent_forms(cov, x, Um, Vm, context=ctx)
    h = 1e-6
    for nm, value in cov.get_params().items():
        up, down = (ab.SquaredExponential(1.0, 1.0) + ab.SquaredExponential(1.0, 1.0) * ab.Constant(0.5) + ab.IndependentNoise(0.1)
                    for _ in range(2))
        up.set_param(nm, value + h)
        down.set_param(nm, value - h)
        dK = (ctx.gram(up, x) - ctx.gram(down, x)) / (2 * h)
        want = np.sum(Um * (dK @ Vm), axis=0)
        scale = np.sum(np.abs(Um) * (np.abs(dK) @ np.abs(Vm)), axis=0)
        assert np.all(np.abs(got[nm] - want) <= 1e-7 * scale + 1e-9), (nm, got[nm], want)


def test_statuses_and_empty_calls(ctx):
    case = tc.form_case("scaling", 65, 2)
    P = len(case.slots)
    for empty in (dict(ncols=0), dict(n_slots=0)):
        st, _, buf, _ = tc.run_forms(ctx, case, **empty)
        assert st == capi.AGP_OK and gp.all_canary(buf), empty
    bad_node = [(99, 0)] + case.slots[1:]
    inner = [(len(case.nodes) - 1, 0)] + case.slots[1:]  # the root of the tree: not a leaf
    leaf = next(node for node, _ in case.slots if case.nodes[node]["op"] != capi.OP_SCALING)  # (a scaling slot names any tangent column)
    bad_param = [(leaf, 7)] + case.slots[1:]
    for bad in (dict(slots=bad_node), dict(slots=inner), dict(slots=bad_param), dict(n_slots=-1), dict(n_slots=capi.MAX_GRADIENT_SLOTS + 1),
                dict(ldu=case.n - 1), dict(ldv=case.n - 1), dict(ldt=case.n - 1), dict(ldf=case.ncols - 1), dict(ncols=-1)):
        st, _, buf, _ = tc.run_forms(ctx, case, **bad)
        assert st == capi.AGP_ERR_INVALID_ARGUMENT and gp.all_canary(buf), bad
    st, _, buf, _ = tc.run_forms(ctx, case, location=2)
    assert st == capi.AGP_ERR_INVALID_ARGUMENT and gp.all_canary(buf)
    with pytest.raises(ValueError):
        ab.gram_tangent_forms(ab.SquaredExponential(1., 1.), [ab.LinearCombination([0.7, 2.9], [1., -1.])], np.ones(1), np.ones(1), context=ctx)
    # a NaN coordinate: AGP_ERR_NAN_INPUT, nothing written
    cov = ab.SquaredExponential(1., 1.)
    x = np.random.default_rng(1).uniform(0., 4., (65, 3))
    x[7, 1] = np.nan
    with pytest.raises(ab.NanInputError):
        ab.gram_tangent_forms(cov, x, np.ones(65), np.ones(65), context=ctx)
    assert P == len(cc.slot_table(case.cov)) and C.sizeof(capi.GradientSlot) == 8
