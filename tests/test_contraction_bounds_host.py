"""The bound of tests/contraction_cases.py is sound and it bites, before any GPU is involved.

  * The restatement is right: its values agree with the oracle's Gram matrix under the parity bar of tests/test_gram_gpu.py
    for every tree, and its analytic tangents agree with a Richardson-extrapolated central difference of its own
    longdouble values (steps h and h / 2, h = 1e-4 max(1, |theta|)) to 1e-9 |dk|* for every slot of every tree; the
    AGP_OP_SCALING slots through a perturbed Elevation.
  * The bound is sound: an fp64 numpy contraction that adds in the kernel's order (lane, wave, tile, reduce_partials, the
    sparse combination) stays within HALF of it on every case the GPU file runs.
  * The bound bites: each fault below, put into that fp64 restatement, misses the bound on at least one case of every
    family it can occur in.
        drop_row       one pair dropped at the last valid row of a tile
        drop_col       one pair dropped at its last valid column
        diag_twice     the off-diagonal factor 2 applied to the diagonal pairs
        strict_lower   jl > il replaced by jl >= il
        row_major      mode 0 tile ids decoded row-block-major
        wrong_ld       group slab g read with group g + 1's leading dimension
        next_tangent   the tangent column of the next slot used for an AGP_OP_SCALING slot
        zero_branch    the product rule's zero branch returning tl * r + l * tr
        meas_tangent   a MeasurementOnly gate zeroing the value but not the tangents
        phantom_pair   one phantom diagonal pair contracted in the ragged batch
        m52_third      a Matern-5/2 tangent with 1/3 replaced by 0.333
    zero_branch: for finite operands the two branches are the same number (l == 0 makes l * tr vanish), so this fault can
    only show where the right operand is not finite.  That is the case the short circuit exists for - 0 * inf - and the
    'far:noise*se' tree of every family holds it: a point whose squared distance overflows makes the squared
    exponential's length-scale tangent 0 * inf = NaN under a noise factor that is exactly 0; the faulty branch hands the
    NaN on (miss factor inf).
  * The input conditions of the cases module hold for every case.
No GPU."""
import copy

import numpy as np
import pytest

import albatross_amd as ab  # noqa: F401  (the package must import without a GPU)
from albatross_amd import _capi as capi
from oracle import oracle_py as orc

import contraction_cases as cc
import gram_path_cases as gp

LD = cc.LD
FAMILIES = cc.SYM_FAMILIES + ["sparse_rect", "sparse_groups", "batched"]
DENSE_SCALE = {"dense_nll": 0.5, "dense_loo": 1.0}


def family_cases(family, small=False):
    """every single-contraction case of a family (the batched family: its problems, [(case, phantom tiles)])"""
    if family in cc.SYM_FAMILIES:
        out = [cc.symmetric_case(family, **s) for s in cc.symmetric_specs(family)]
    elif family == "sparse_rect":
        out = [cc.rect_case(**s) for s in cc.rect_specs()]
    elif family == "sparse_groups":
        out = [cc.group_case(**s) for s in cc.group_specs()]
    else:
        out = [cc.cut_slots(c, ns) for loo in (False, True) for b in cc.BATCHES for c, ns in cc.batch_problems(b, loo)]
    return [c for c in out if not small or c.fr.n <= 330]


def phantom_tiles(family, case):
    return cc.lower_tiles(cc.N_PAD) - case.tiles if family == "batched" else 0


def final_scale(case):
    return DENSE_SCALE.get(case.family, 1.0)


def test_longdouble_is_wider_than_double():
    assert cc.HAVE_LONGDOUBLE


def test_bound_constants():
    """the counts of the derivation, spelled out"""
    assert cc.d_sum(1) == 39 and cc.d_sum(300) == 40 and cc.d_sum(257, combination=True) == 43
    se = dict(op=cc.SE, metric=capi.METRIC_EUCLIDEAN, order=0)
    assert cc.c_leaf(se, 3, 32.) == 3 + 32 * 11 + 15 and cc.c_leaf(se, 1, 32.) == 3 + 32 * 3 + 7
    m52 = dict(op=cc.M52, metric=capi.METRIC_ANGULAR, order=0)
    assert cc.c_leaf(m52, 3, 8.) == 3 + 8 * 6 + 26
    assert cc.c_leaf(dict(op=capi.OP_POLYNOMIAL, order=3), 1, 0.) == 8 and cc.c_leaf(dict(op=capi.OP_SCALING), 1, 0.) == 3


def test_integer_directions():
    d = cc.integer_directions()
    assert len(d) >= 100
    norms = np.sqrt((d * d).sum(axis=1))
    assert np.all(norms == np.round(norms)) and set(norms) <= {3., 7., 9., 11.}
    c = (d @ d.T) / np.outer(norms, norms)
    exact = (np.abs(c) == 1.)
    assert np.all(np.abs(c[~exact]) <= 0.99) and exact.sum() > len(d)  # the diagonal and the antipodes


def _tree_pairs(name):
    """the feature pairs a tree's restatement is checked on: a symmetric set of 33 points with ids and a plain x measurement
    rectangle"""
    c1 = cc.symmetric_case("sparse_sym", name, 33, ids=True)
    c2 = cc.rect_case(name, 17, 35, meas=(False, True))
    c3 = cc.rect_case(name, 17, 35, meas=(True, True), ids="rows")
    return [c1, c2, c3]


@pytest.mark.parametrize("name", cc.TREE_NAMES)
def test_restatement_values_match_the_oracle(name):
    for c in _tree_pairs(name):
        _, _, v, _ = cc.eval_tangent(c.nodes, c.slots, c.fr, c.fc, c.tr, c.tc)
        want = orc.gram(c.cov, c.fr, c.fc, x_meas=c.fr.is_measurement, y_meas=c.fc.is_measurement)
        assert gp.close(np.asarray(v, dtype=np.float64), want), c.name


def _values(case, nodes, fr, fc):
    return cc.eval_tangent(nodes, [], fr, fc)[2]


def _perturbed(case, slot, delta):
    """(nodes, fr, fc) with the parameter of slot (node, param, name) moved by delta; an AGP_OP_SCALING slot moves the
    parameter of its scaling function and re-evaluates the scale columns"""
    node, param, name = slot
    nodes = copy.deepcopy(case.nodes)
    if nodes[node]["op"] != capi.OP_SCALING:
        nodes[node]["params"][param] += delta
        return nodes, case.fr, case.fc
    cov = copy.deepcopy(case.cov)
    fn = cov.param_slots()[1][param][0]
    fn.set_param(name, fn.get_params()[name] + delta)
    sets = [gp.features(cov, f.coords, meas=f.is_measurement, ids=f.eq_id) for f in (case.fr, case.fc)]
    return nodes, sets[0], sets[1]


@pytest.mark.parametrize("name", cc.TREE_NAMES)
def test_analytic_tangents_match_richardson(name):
    worst = 0.
    for c in _tree_pairs(name):
        table, columns = c.cov.param_slots()
        assert [(n_, p_) for n_, p_, _ in table] == c.slots
        dk, dka, _, _ = cc.eval_tangent(c.nodes, c.slots, c.fr, c.fc, c.tr, c.tc)
        for g, slot in enumerate(table):
            node, param, pname = slot
            theta = c.nodes[node]["params"][param] if c.nodes[node]["op"] != capi.OP_SCALING else columns[param][0].get_params()[pname]
            h = LD(1e-4) * max(1., abs(theta))

            def central(step):
                up, dn = _perturbed(c, slot, float(step)), _perturbed(c, slot, -float(step))
                # the step that was actually taken, in the parameter's float64
                return (_values(c, *up) - _values(c, *dn)) / (LD(theta + float(step)) - LD(theta - float(step)))
            fd = (4 * central(h / 2) - central(h)) / 3
            err = np.abs(fd - dk[g])
            tol = LD(1e-9) * dka[g]
            assert np.all(err <= tol), (c.name, slot, float(np.max(err - tol)))
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.max(np.where(err == 0, 0, err / dka[g]))))
    print(f"{name}: worst |analytic - richardson| / |dk|* {worst:.3g}")


@pytest.mark.parametrize("family", FAMILIES)
def test_input_conditions_hold(family):
    for c in family_cases(family):
        cc.check_inputs(c)
        t = cc.reference(c)[2]
        assert t <= c.t_cap
    caps = [c.t_cap for c in family_cases(family)]
    print(f"{family}: {len(caps)} cases, largest exponent argument assumed by c_eval {min(caps):g} .. {max(caps):g}")


@pytest.mark.parametrize("family", FAMILIES)
def test_fp64_in_kernel_order_meets_half_the_bound(family):
    worst, worst_name, worst_combo = 0., "", 0.
    for c in family_cases(family):
        ref, scale, _, _ = cc.reference(c)
        sc = final_scale(c)
        sums = cc.kernel_order_sum(c, sc, phantom_tiles=phantom_tiles(family, c))
        tiles = c.tiles + phantom_tiles(family, c)
        gamma = (cc.d_sum(tiles) + cc.c_eval(c.nodes, c.dim, c.t_cap)) * cc.U
        r = cc.ratio(sums, sc * ref, gamma * abs(sc) * scale)
        if r > worst:
            worst, worst_name = r, c.name
        assert r <= 0.5, (c.name, r)
        if family.startswith("sparse"):
            for which in range(3):
                col = np.arange(len(c.slots)) % cc.GRAD_GROUP  # the other sets are the same for every slot group
                others = [cc.reduce_partials(o)[col] for o in cc.sparse_others(c, which)]
                got = cc.combination(sums, which, others)
                oref = [np.sum(o.astype(LD), axis=0)[col] for o in cc.sparse_others(c, which)]
                oabs = [np.sum(np.abs(o), axis=0)[col] for o in cc.sparse_others(c, which)]
                cref = cc.combination(ref, which, oref)
                cscale = -cc.combination(scale, which, oabs)
                rc = cc.ratio(got, cref, c.gamma(combination=True) * cscale)
                worst_combo = max(worst_combo, rc)
                assert rc <= 0.5, (c.name, which, rc)
    print(f"{family}: fp64 in kernel order, worst error / bound {worst:.3g} ({worst_name})"
          + (f", three-way combination {worst_combo:.3g}" if family.startswith("sparse") else ""))


LOWER = cc.SYM_FAMILIES + ["sparse_groups", "batched"]
EVERY = FAMILIES
FAULTS = {
    "drop_row": EVERY, "drop_col": EVERY, "diag_twice": LOWER, "strict_lower": LOWER, "row_major": ["sparse_rect"],
    "wrong_ld": ["sparse_groups"], "next_tangent": EVERY, "zero_branch": EVERY, "meas_tangent": EVERY, "phantom_pair": ["batched"],
    "m52_third": EVERY,
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_fault_misses_the_bound(fault):
    for family in FAULTS[fault]:
        misses = []
        for c in family_cases(family, small=True):
            if not c.slots:
                continue
            ref, scale, _, _ = cc.reference(c)
            sc = final_scale(c)
            ph = phantom_tiles(family, c)
            if fault == "phantom_pair":
                # a row behind n_b read as the problem's first feature, under the weight of diag(C_b, I) and alpha = 0: 1
                dk00 = np.array([d[0, 0] for d in cc.block_tangents(c, c.blocks[0], np.float64)[0]])
                got = sc * (cc.reduce_partials(cc.kernel_order_partials(c, phantom_tiles=ph)) + 1.0 * dk00)
            else:
                got = cc.kernel_order_sum(c, sc, mut=(fault,), phantom_tiles=ph)
            gamma = (cc.d_sum(c.tiles + ph) + cc.c_eval(c.nodes, c.dim, c.t_cap)) * cc.U
            r = cc.ratio(got, sc * ref, gamma * abs(sc) * scale)
            if r > 1.:
                misses.append((r, c.name))
        assert misses, (fault, family)
        r, name = min(misses)
        print(f"{fault} / {family}: misses the bound on {len(misses)} cases, smallest miss factor {r:.3g} ({name})")
