"""CPU tests (no GPU) of agp_logo_nll_gradient_batch: the header and the binding, the pooled plan of the groups of all
problems (csrc/logo_batch_plan.h through agp_debug_logo_batch_plan, which needs no context) against a numpy restatement,
and the phantom-row argument the entry rests on: problem b padded to diag(K_b, I) with groups on real rows only has the
value and gradient of the problem on its own points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from albatross_amd import _capi as capi
from test_logo_gradient_host import PARAMS, groupings, logo_closed_form, _problem
from test_logo_marginal_host import logo_marginal_closed_form
from test_loo_gradient_host import se_gram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_capi_binds_it():
    text = open(os.path.join(ROOT, "include", "albatross_amd.h")).read()
    assert re.search(r"AGP_API int agp_logo_nll_gradient_batch\(agp_context \*ctx, int count,"
                     r"\s*const agp_kernel \*const \*kernels, const agp_features \*const \*features,"
                     r"\s*const double \*y, int64_t ldy,\s*const double \*y_var, int64_t ldv,\s*const int64_t \*n_groups,"
                     r"\s*const int64_t \*const \*offsets, const int64_t \*const \*indices,\s*int predict_type,"
                     r"\s*const int \*n_slots,\s*const agp_gradient_slot \*const \*slots,"
                     r"\s*const double \*const \*tangents, int64_t ldt,\s*double \*logo_nll,"
                     r"\s*double \*grad_logo_nll, int64_t ldg,\s*double \*mean_weights, int64_t ldw,"
                     r"\s*double \*const \*group_nll,\s*int \*status\);", text)
    assert "composition" in text  # a problem's bits may depend on the composition of the batch
    exports = {name: (res, args) for name, res, args in capi.EXPORTS}
    ragged = exports["agp_loo_nll_gradient_batch_ragged"][1]
    P, i64 = ragged[0], C.c_int64
    # the ragged leave-one-out arguments with the groups and the predict type before n_slots and group_nll before status
    assert exports["agp_logo_nll_gradient_batch"] == (C.c_int, ragged[:8] + [P, P, P, C.c_int] + ragged[8:17] + [P, P])
    assert i64 in ragged


# ---- the pooled plan ------------------------------------------------------------------------------------------------
def _plan(sizes, groups, cols_max=0):
    """agp_debug_logo_batch_plan on groups[b] = list of index lists; (rc, record as a dict)"""
    lib = capi.load_debug()
    count = len(sizes)
    offs, inds = [], []
    for gs in groups:
        offs.append(np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64))
        inds.append(np.asarray([i for g in gs for i in g], dtype=np.int64))
    n = np.asarray(sizes, dtype=np.int64)
    ng = np.asarray([len(gs) for gs in groups], dtype=np.int64)
    op = (C.c_void_p * count)(*[o.ctypes.data for o in offs])
    ip = (C.c_void_p * count)(*[i.ctypes.data if len(i) else None for i in inds])
    words = C.c_int64(0)
    rc = lib.agp_debug_logo_batch_plan(count, n.ctypes.data, ng.ctypes.data, op, ip, cols_max, None, 0, C.byref(words))
    if rc != capi.AGP_OK:
        return rc, None
    out = np.zeros(words.value, dtype=np.int64)
    assert lib.agp_debug_logo_batch_plan(count, n.ctypes.data, ng.ctypes.data, op, ip, cols_max, out.ctypes.data, len(out),
                                         C.byref(words)) == capi.AGP_OK
    T, K = int(out[0]), int(out[1])
    at = 6
    chunks = out[at:at + 4 * K].reshape(K, 4); at += 4 * K
    terms = out[at:at + 3 * T].reshape(T, 3); at += 3 * T
    idx = []
    for m, cnt, _, _ in chunks:
        idx.append(out[at:at + m * cnt].reshape(cnt, m)); at += m * cnt
    csr_off = out[at:at + count + 1]; at += count + 1
    csr_terms = out[at:at + T]; at += T
    assert at == len(out)
    return rc, dict(terms=terms, chunks=chunks, idx=idx, csr_off=csr_off, csr_terms=csr_terms, cols_max=int(out[2]),
                    groups_max=int(out[3]), img_max=int(out[4]))


def _random_groups(rng, n):
    """a ragged grouping of some of the n points: random sizes, some empty groups, some points in no group"""
    perm = rng.permutation(n)
    groups, at = [], 0
    while at < n and rng.random() > 0.03:
        m = int(min(n - at, rng.choice([0, 1, 1, 2, 3, 4, 7, 16, 33, 64, 130])))
        groups.append(perm[at:at + m].tolist())
        at += m
    return groups


@pytest.mark.parametrize("count", range(1, 13))
def test_pooled_plan_against_numpy(count):
    rng = np.random.default_rng(100 + count)
    sizes = rng.integers(1, 400, count).tolist()
    groups = [_random_groups(rng, n) if rng.random() > 0.15 else [] for n in sizes]
    cols_max = 0 if count % 3 else 300  # also a bound that splits size classes
    rc, p = _plan(sizes, groups, cols_max)
    assert rc == capi.AGP_OK
    # numpy restatement: the non-empty groups sorted by (size, problem, group)
    want = sorted((len(g), b, j) for b, gs in enumerate(groups) for j, g in enumerate(gs) if len(g))
    assert [(int(s), int(b), int(j)) for b, j, s in p["terms"]] == want
    assert p["cols_max"] == (cols_max or count * max(sizes))
    at = 0
    for (m, cnt, term_off, img), idx in zip(p["chunks"], p["idx"]):
        assert term_off == at and cnt >= 1
        mine = want[at:at + cnt]
        sz = [s for s, _, _ in mine]
        assert m == max(sz) and m <= 2 * min(sz)
        assert cnt <= p["groups_max"] and cnt * img <= p["img_max"]
        assert cnt == 1 or cnt * m <= p["cols_max"]
        for row, (s, b, j) in zip(idx, mine):  # every group with its own indices in the caller's order, then padding
            assert row[:s].tolist() == groups[b][j] and (row[s:] == -1).all()
        # greedy: the next group would have broken a limit
        if at + cnt < len(want):
            s_next = want[at + cnt][0]
            img_next = img // ((m + 127) // 128) * ((s_next + 127) // 128)  # images are per 128-row diagonal block
            assert (s_next > 2 * min(sz) or cnt + 1 > p["groups_max"] or (cnt + 1) * s_next > p["cols_max"]
                    or (cnt + 1) * img_next > p["img_max"])
        at += cnt
    assert at == len(want)
    # the per-problem term lists partition the terms, each ascending
    assert p["csr_off"][0] == 0 and p["csr_off"][-1] == len(want)
    assert sorted(p["csr_terms"].tolist()) == list(range(len(want)))
    for b in range(count):
        mine = p["csr_terms"][p["csr_off"][b]:p["csr_off"][b + 1]].tolist()
        assert mine == [q for q, (_, pb, _) in enumerate(want) if pb == b]


def test_singletons_of_eight_problems_are_two_chunks():
    """4096 singletons against the image bound of one chunk (256 MiB of images: 3640 groups of at most 128 points)"""
    rc, p = _plan([512] * 8, [[[i] for i in range(512)]] * 8)
    assert rc == capi.AGP_OK
    assert p["chunks"][:, :3].tolist() == [[1, 3640, 0], [1, 456, 3640]]


def test_plan_refuses_malformed_groups():
    sizes = [10, 6, 8]
    good = [[[0, 1], [5]], [[2, 3, 4]], [[7], []]]
    assert _plan(sizes, good)[0] == capi.AGP_OK

    def refused(b, gs):
        bad = [list(g) for g in good]
        bad[b] = gs
        assert _plan(sizes, bad)[0] == capi.AGP_ERR_INVALID_ARGUMENT

    refused(1, [[2, 3, 2]])       # twice in one group
    refused(0, [[0, 1], [1]])     # in two groups
    refused(1, [[2, 3, 6]])       # n_b = 6: out of range although below the padded size 10
    refused(1, [[2, 3, 9]])
    refused(2, [[7], [-1]])
    refused(2, [[8]])
    assert _plan([10, 0], [[[1]], []])[0] == capi.AGP_ERR_INVALID_ARGUMENT  # a size <= 0
    # malformed offsets, handed in directly
    lib = capi.load_debug()
    n = np.array([10], dtype=np.int64)
    ng = np.array([2], dtype=np.int64)
    ind = np.arange(5, dtype=np.int64)
    words = C.c_int64(0)
    for off in ([1, 3, 5], [0, 3, 2]):
        o = np.array(off, dtype=np.int64)
        rc = lib.agp_debug_logo_batch_plan(1, n.ctypes.data, ng.ctypes.data, (C.c_void_p * 1)(o.ctypes.data),
                                           (C.c_void_p * 1)(ind.ctypes.data), 0, None, 0, C.byref(words))
        assert rc == capi.AGP_ERR_INVALID_ARGUMENT


# ---- phantom rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closed_form", [logo_closed_form, logo_marginal_closed_form])
@pytest.mark.parametrize("grouping", ["ragged", "fours", "one", "singletons"])
def test_block_diagonal_padding_changes_nothing(grouping, closed_form):
    """diag(K_b, I) with zero targets and zero variances on the phantom rows and groups on real rows only: the value, u and
    alpha on the real rows and the weight's real block are those of K_b alone, and the weight couples no phantom row to a
    real one - so the contraction over the real pairs is the problem's own gradient"""
    n, pad = 40, 13
    x, y, s = _problem(n, True)
    K, dK = se_gram(x, PARAMS)
    K = K + np.diag(s)
    groups = groupings(n)[grouping]
    alone = closed_form(K, y, s, groups)
    Kp = np.eye(n + pad)
    Kp[:n, :n] = K
    padded = closed_form(Kp, np.concatenate([y, np.zeros(pad)]), np.concatenate([s, np.zeros(pad)]), groups)
    assert abs(padded[0] - alone[0]) <= 1e-13 * abs(alone[0])
    W, Wp = alone[1], padded[1]
    scale = np.abs(W).max()
    assert np.abs(Wp[:n, :n] - W).max() <= 1e-12 * scale
    assert np.abs(Wp[n:, :]).max() <= 1e-12 * scale  # S = C B C is diag(S_b, 0) and u, alpha vanish on phantom rows
    for k in (2, 3):  # u and alpha
        assert np.abs(padded[k][:n] - alone[k]).max() <= 1e-12 * np.abs(alone[k]).max()
        assert np.abs(padded[k][n:]).max() == 0.
    for d in dK:
        # (entries agree to 1e-12 scale, so the contractions agree to that times sum |dK|)
        assert abs(np.sum(Wp[:n, :n] * d) - np.sum(W * d)) <= 1e-12 * scale * np.abs(d).sum()
