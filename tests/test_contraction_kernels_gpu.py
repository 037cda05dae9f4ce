"""The gradient contraction kernels on their own, on the caller's weights: nll_grad_contract_kernel<DIMP, LOO> with
nll_grad_reduce_kernel (agp_debug_contract_dense), nll_grad_contract_batched_kernel<DIMP, LOO> with
nll_grad_reduce_batched_kernel on ContractDesc records (agp_debug_contract_batched) and sparse_contract_kernel<DIMP> in its
three modes with sparse_grad_reduce_kernel (agp_debug_contract_sparse) - the launchers of csrc/contract_internal.h, which the
gradient entries call too (csrc/debug_api.hip).

Cases, reference, scale and bound are tests/contraction_cases.py's (its docstring derives the bound;
tests/test_contraction_bounds_host.py shows that plain fp64 in the kernel's order stays within half of it and that eleven
kinds of fault do not).  Every test asserts error / bound <= 1 against the longdouble reference and prints the worst ratio;
what a kernel must not read is NaN (the weight's upper triangle and padding rows, the tangent buffer beyond n and beyond the
columns in use, u without LOO) and what it must not write is compared bit for bit (out beyond n_slots, the partials beyond the
tiles and of unused slot groups); two calls give the same bits."""
import numpy as np
import pytest

import contraction_cases as cc
import gram_path_cases as gp

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not cc.HAVE_LONGDOUBLE, reason="np.longdouble is no wider than float64 here: no reference")]

INVALID_ARGUMENT = 1  # include/albatross_amd.h: AGP_ERR_INVALID_ARGUMENT
GG = cc.GRAD_GROUP
WORST = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def note(test, case, r):
    WORST[test] = max(WORST.get(test, 0.), r)
    print(f"{case}: worst error / bound {r:.3g} (so far in {test}: {WORST[test]:.3g})")


def check_partial(partial, tiles, n_slots):
    """the partials of the last slot group: finite, zero in the columns of unused slots, canaries behind the tiles"""
    last = n_slots - (n_slots - 1) // GG * GG if n_slots else 0
    if n_slots == 0:
        assert gp.all_canary(partial)
        return
    assert np.all(np.isfinite(partial[:tiles]))
    assert np.all(partial[:tiles, last:] == 0.)
    assert gp.all_canary(partial[tiles:])


def _sym_id(spec):
    return ":".join(f"{k}={v}" for k, v in sorted(spec.items()))


DENSE = [(f, s) for f in ("dense_nll", "dense_loo") for s in cc.symmetric_specs(f)]


@pytest.mark.parametrize("family,spec", DENSE, ids=[f"{f}:{_sym_id(s)}" for f, s in DENSE])
def test_dense(ctx, family, spec):
    case = cc.symmetric_case(family, **spec)
    loo = family == "dense_loo"
    G, tiles = len(case.slots), case.tiles
    ref, scale, _, _ = cc.reference(case)
    sc = 1.0 if loo else 0.5
    st, out, partial = cc.run_dense(ctx, case, loo, sc)
    assert st == 0, st
    r = cc.ratio(out[:G], sc * ref, case.gamma() * sc * scale)
    note("test_dense", case.name, r)
    assert r <= 1., (case.name, r)
    assert gp.all_canary(out[G:])
    check_partial(partial, tiles, G)
    st2, out2, partial2 = cc.run_dense(ctx, case, loo, sc)
    assert st2 == 0 and same_bits(out, out2) and same_bits(partial, partial2)
    # the scale multiplies exactly
    _, one, _ = cc.run_dense(ctx, case, loo, 1.0)
    _, half, _ = cc.run_dense(ctx, case, loo, -0.5)
    assert same_bits(half[:G], -0.5 * one[:G]) and gp.all_canary(half[G:])
    if not loo:  # u went in full of NaN: it is not read, and a finite one changes no bit
        _, out3, _ = cc.run_dense(ctx, case, False, sc, u=case.u)
        assert same_bits(out, out3)


SPARSE = ([("sparse_sym", s) for s in cc.symmetric_specs("sparse_sym")] + [("sparse_rect", s) for s in cc.rect_specs()]
          + [("sparse_groups", s) for s in cc.group_specs()])


def _sparse_case(family, spec):
    if family == "sparse_sym":
        return cc.symmetric_case(family, **spec)
    return cc.rect_case(**spec) if family == "sparse_rect" else cc.group_case(**spec)


@pytest.mark.parametrize("family,spec", SPARSE, ids=[f"{f}:{_sym_id(s)}" for f, s in SPARSE])
def test_sparse(ctx, family, spec):
    case = _sparse_case(family, spec)
    G, tiles = len(case.slots), case.tiles
    ref, scale, _, _ = cc.reference(case)
    which = case.seed % 3
    st, out, combo, partial = cc.run_sparse(ctx, case, which)
    assert st == 0, st
    r = cc.ratio(out[:G], ref, case.gamma() * scale)
    col = np.arange(G) % GG
    others = cc.sparse_others(case, which)
    cref = cc.combination(ref, which, [np.sum(o.astype(cc.LD), axis=0)[col] for o in others])
    cscale = -cc.combination(scale, which, [np.sum(np.abs(o), axis=0)[col] for o in others])
    rc = cc.ratio(combo[:G], cref, case.gamma(combination=True) * cscale)
    note(f"test_sparse[{family}]", case.name, max(r, rc))
    assert r <= 1. and rc <= 1., (case.name, r, rc)
    assert gp.all_canary(out[G:]) and gp.all_canary(combo[G:])
    check_partial(partial, tiles, G)
    st2, out2, combo2, partial2 = cc.run_sparse(ctx, case, which)
    assert st2 == 0 and same_bits(out, out2) and same_bits(combo, combo2) and same_bits(partial, partial2)


@pytest.mark.parametrize("loo", [False, True], ids=["nll", "loo"])
@pytest.mark.parametrize("batch", list(cc.BATCHES))
def test_batched(ctx, batch, loo):
    problems = cc.batch_problems(batch, loo)
    sc = 1.0 if loo else 0.5
    st, out, partial, ldo, groups = cc.run_batched(ctx, problems, loo, sc)
    assert st == 0, st
    tiles = cc.lower_tiles(cc.N_PAD)
    count = len(problems)
    rows = out[:ldo * count].reshape(count, ldo)
    assert gp.all_canary(out[ldo * count:])
    parts = partial[:count * groups * tiles * GG].reshape(count, groups, tiles, GG)
    assert gp.all_canary(partial[count * groups * tiles * GG:])
    worst = 0.
    for b, (case, ns) in enumerate(problems):
        single = cc.cut_slots(case, ns)
        ref, scale, _, _ = cc.reference(single)
        gamma = (cc.d_sum(tiles) + cc.c_eval(single.nodes, single.dim, single.t_cap)) * cc.U
        worst = max(worst, cc.ratio(rows[b, :ns], sc * ref, gamma * sc * scale))
        assert gp.all_canary(rows[b, ns:]), (batch, b)
        # bit for bit the single-problem entry's value
        st1, one, _ = cc.run_dense(ctx, single, loo, sc)
        assert st1 == 0 and same_bits(rows[b, :ns], one[:ns]), (batch, b, rows[b, :ns], one[:ns])
        used = -(-ns // GG)
        real = case.tiles  # the lower tiles of n_b rows come first in the enumeration of the padded size
        assert np.all(np.isfinite(parts[b, :used, :real]))
        assert np.all(parts[b, :used, real:] == 0.) and not np.any(np.signbit(parts[b, :used, real:])), (batch, b)  # phantom tiles
        assert gp.all_canary(parts[b, used:]), (batch, b)  # slot groups the problem does not have
    note("test_batched", f"{batch}:{'loo' if loo else 'nll'}", worst)
    assert worst <= 1., (batch, worst)
    st2, out2, partial2, _, _ = cc.run_batched(ctx, problems, loo, sc)
    assert st2 == 0 and same_bits(out, out2) and same_bits(partial, partial2)


def test_bad_extents_are_refused(ctx):
    d = cc.symmetric_case("dense_nll", "scaling", 65)
    n, G = d.fr.n, len(d.slots)
    for bad in (dict(ldc=n - 1), dict(c_elems=d.ld * (n - 1) + n - 1), dict(ldt=n - 1), dict(tang_elems=d.ldt + n - 1),
                dict(out_elems=G - 1), dict(partial_elems=GG * cc.lower_tiles(n) - 1), dict(n_slots=-1), dict(n_slots=65)):
        st, out, partial = cc.run_dense(ctx, d, False, 0.5, **bad)
        assert st == INVALID_ARGUMENT, bad
        assert gp.all_canary(out) and gp.all_canary(partial)
    probs = cc.batch_problems("scaling", False)
    for bad in (dict(n_pad=129), dict(ldo=5), dict(out_elems=8), dict(partial_elems=10)):
        st = cc.run_batched(ctx, probs, False, 0.5, **bad)[0]
        assert st == INVALID_ARGUMENT, bad
    r = cc.rect_case("scaling", 63, 65)
    for bad in (dict(ldw=62), dict(w_elems=r.ld * 64 + 62), dict(ldtr=62), dict(ldtc=64), dict(tc_elems=10), dict(mode=1), dict(mode=3),
                dict(which=3), dict(out_elems=G - 1), dict(combo_elems=G - 1), dict(partial_elems=GG * 2 - 1)):
        assert cc.run_sparse(ctx, r, **bad)[0] == INVALID_ARGUMENT, bad
    g = cc.group_case("scaling", "ragged")
    off, wld, woff = g.off.copy(), g.wld.copy(), g.woff.copy()
    off[-1] += 1
    wld[3] = cc.GROUP_SIZES[3] - 1
    woff[-1] = g.wflat.size - 3
    empty = g.off.copy()
    empty[2] = empty[1]
    for bad in (dict(off=off), dict(wld=wld), dict(woff=woff), dict(off=empty), dict(G=0), dict(mode=0), dict(partial_elems=GG * g.tiles - 1)):
        assert cc.run_sparse(ctx, g, **bad)[0] == INVALID_ARGUMENT, bad
