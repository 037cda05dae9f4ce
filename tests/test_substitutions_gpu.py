"""Every triangular substitution path of csrc/solve.hip on its own, through agp_debug_substitute (csrc/debug_api.hip):
the multi-RHS forward / backward / right solves on the MFMA and their batched forms, the look-ahead on two streams, the
vector chains on explicitly inverted 128 x 128 blocks, back_update_kernel, the batched vector solve and the one-launch
backward substitution in both hand-over modes and batched.

Shapes, matrices, right-hand sides and the bound are tests/substitution_cases.py's (its docstring derives the bound;
tests/test_substitution_bounds_host.py shows a plain restatement of each path meets it on these very inputs).  Each case
asserts residual / bound <= 1 against the factor the device solved with, and memory safety bit for bit: the NaN padding
rows of ldb > rows, the NaN columns beyond m, the NaN gaps between the problems of a batch, and - with rhs_lower - the
entries of the right-hand side above its block diagonal (NaN where the solve never reads, zeros where it does) all come
back unchanged."""
import ctypes as C

import numpy as np
import pytest

from albatross_amd import _capi as capi
import substitution_cases as sc

pytestmark = pytest.mark.gpu

NB = sc.NB
NAN_BITS = np.array(np.nan).view(np.uint64)
SENTINEL_BITS = np.uint64(0xFFF8A5A5DEADBEEF)  # csrc/pub.h: PUB_SENTINEL
INVALID_ARGUMENT = 1  # include/albatross_amd.h: AGP_ERR_INVALID_ARGUMENT
EXTRA_COLS = 2
CASES = sc.all_cases()


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pick_ld(rows):
    """A leading dimension > rows that the factor's own (a multiple of 8: api.hip, factor_ld) never equals."""
    ld = rows + 3
    return ld + 2 if ld % 8 == 0 else ld


def substitute(ctx, kind, Ks, buf, rows, cols, ldb, stride_B=0, lda=0, opt=0, want_W=False):
    """agp_debug_substitute on the padded buffer `buf` (in place).  Returns (status, flags, factors, inverted blocks)."""
    fn = capi.load_debug().agp_debug_substitute
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int64] * 3 + [C.c_void_p] + [C.c_int64] * 6 + [C.c_void_p] * 3
    n, count = Ks[0].shape[0], len(Ks)
    Kall = np.concatenate([np.asarray(K).ravel(order="F") for K in Ks])
    Lall = np.zeros(count * n * n)
    flags = np.full(2 * count, -1, dtype=np.int32)
    W = np.full(-(-n // NB) * NB * NB, np.nan) if want_W else None
    st = fn(ctx._h, kind, _p(Kall), n, count, lda, _p(buf), buf.size, rows, cols, ldb, stride_B, opt, _p(flags), _p(Lall), _p(W))
    Ls = [np.tril(Lall[p * n * n:(p + 1) * n * n].reshape((n, n), order="F")) for p in range(count)]
    return st, flags, Ls, W


def padded(M, ld, stride=None, extra_cols=EXTRA_COLS):
    """M (rows x cols) in a NaN-filled column-major buffer of leading dimension ld with extra_cols further columns (and up
    to `stride` doubles): (flat buffer, view of the rows x cols part)."""
    rows, cols = M.shape
    size = ld * (cols + extra_cols)
    flat = np.full(max(size, stride or 0), np.nan)
    view = flat[:size].reshape((ld, cols + extra_cols), order="F")
    view[:rows, :cols] = M
    return flat, view


def check_padding(flat, view, rows, cols):
    """Everything outside the rows x cols part is still the NaN it was, bit for bit."""
    size = view.size
    assert np.all(_bits(view[rows:, :]) == NAN_BITS), "padding rows written"
    assert np.all(_bits(view[:, cols:]) == NAN_BITS), "columns beyond m written"
    assert np.all(_bits(flat[size:]) == NAN_BITS), "gap behind the slab written"


def as_left(kind, M):
    """The n x cols matrix of the equivalent left solve (the right-hand forms hold its transpose)."""
    return M.T if kind in (sc.RIGHT_LT, sc.RIGHT_LT_BATCHED) else M


def run_single(ctx, case, rhs_lower=None, lda=None):
    """One unbatched case: (X as the left-solve matrix, L, B, flags)."""
    kind, n, cols = case["kind"], case["n"], case["cols"]
    B = sc.case_rhs(case)
    stored = B.T if kind == sc.RIGHT_LT else B
    if kind in (sc.FWD_MAT, sc.FWD_MAT_LOOKAHEAD) and case["lower"]:
        stored = stored.copy()
        stored[sc.untouched_above(n, cols, sc.NBO)[0]] = np.nan  # never read, never written under rhs_lower
    rows_s, cols_s = stored.shape
    ldb = pick_ld(rows_s)
    flat, view = padded(stored, ldb)
    lower = (1 if case["lower"] else 0) if rhs_lower is None else rhs_lower
    if not lower:
        view[:rows_s, :cols_s] = B.T if kind == sc.RIGHT_LT else B
    st, flags, Ls, W = substitute(ctx, kind, sc.case_matrices(case), flat, rows_s, cols_s, ldb, opt=lower,
                                  lda=case.get("lda", 0) if lda is None else lda, want_W=kind in (sc.FWD_VEC, sc.BWD_VEC))
    assert st == 0, st
    check_padding(flat, view, rows_s, cols_s)
    X = view[:rows_s, :cols_s].copy()
    if lower:
        above, zeros = sc.untouched_above(n, cols, sc.NBO)
        assert np.all(_bits(X[above]) == NAN_BITS), "entries above the block diagonal written under rhs_lower"
        assert np.all(_bits(X[zeros]) == 0), "zeros between a block row's columns and its outer block's written"
        X[above] = 0.0
        assert np.all(X[np.triu_indices(n, 1, cols)] == 0.0), "a lower-triangular right-hand side has a lower-triangular solution"
    return as_left(kind, X), Ls[0], B, flags, W


def run_batched(ctx, case, zero_strides=False):
    """One batched case: ([X_p], [L_p], [B_p], flags).  Strides larger than a slab, NaN in the gaps."""
    kind, n, cols, count = case["kind"], case["n"], case["cols"], case["count"]
    right = kind == sc.RIGHT_LT_BATCHED
    Bs = [sc.case_rhs(case, p) for p in range(count)]
    stored = [(B.T if right else B).copy() for B in Bs]
    lower = 1 if case["lower"] else 0
    if lower:
        for S in stored:
            S[sc.untouched_above(n, cols)[0]] = np.nan
    rows_s, cols_s = stored[0].shape
    vector = cols_s == 1 and not right
    ldb = pick_ld(rows_s)
    extra = 0 if vector else EXTRA_COLS
    slab = ldb * (cols_s + extra)
    stride = 0 if zero_strides else slab + 7
    step = stride if stride else slab
    flat = np.concatenate([padded(S, ldb, stride=stride, extra_cols=extra)[0] for S in stored])
    assert flat.size == count * step
    st, flags, Ls, _ = substitute(ctx, kind, sc.case_matrices(case), flat, rows_s, cols_s, ldb, stride_B=stride, opt=lower,
                                  lda=0 if zero_strides else pick_ld(n) + 1)
    assert st == 0, st
    Xs = []
    for p in range(count):
        part = flat[p * step:(p + 1) * step]  # the slab of problem p and the gap behind it
        v = part[:slab].reshape((ldb, cols_s + extra), order="F")
        check_padding(part, v, rows_s, cols_s)
        X = v[:rows_s, :cols_s].copy()
        if lower:
            above = sc.untouched_above(n, cols)[0]
            assert np.all(_bits(X[above]) == NAN_BITS), "entries above the block diagonal written under rhs_lower"
            X[above] = 0.0
        Xs.append(as_left(kind, X))
    return Xs, Ls, Bs, flags


def check_coop(flags, Xs):
    assert np.all(flags[0::2] == 0), f"hand-over timed out: {flags[0::2]}"
    for X in Xs:
        assert not np.any(_bits(X) == SENTINEL_BITS), "a sentinel is left in x"


def run_case(ctx, case):
    """Checks 1 and 2 of one case (every problem of a batch against its OWN factor); returns the worst ratio."""
    kind = case["kind"]
    b, transposed = sc.BLOCK_WIDTH[kind], kind in sc.TRANSPOSED
    if case["count"] > 1:
        Xs, Ls, Bs, flags = run_batched(ctx, case)
    else:
        X, L, B, flags, W = run_single(ctx, case)
        Xs, Ls, Bs = [X], [L], [B]
        if W is not None:
            check_identity_padding(W, case["n"])
    if kind in (sc.COOP_DIRECT, sc.COOP_FLAGS, sc.COOP_BATCHED):
        check_coop(flags, Xs)
    if kind == sc.FWD_MAT_LOOKAHEAD:
        assert flags[1] == case["two"], "the look-ahead took the other path than the shape is there for"
    assert len({(L[-1, -1], L[case['n'] // 2, 0]) for L in Ls}) == len(Ls)  # distinct factors: a mix-up between problems shows
    ratios = [sc.residual_ratio(L, X, B, b, transposed) for X, L, B in zip(Xs, Ls, Bs)]
    return max(ratios), Xs, Ls, Bs


def check_identity_padding(W, n):
    """Inverted diagonal blocks (invert_diag_blocks / invert_diag_blocks_forward): rows and columns beyond nbk of the last
    block are exactly the identity, and every block is finite."""
    nblk = -(-n // NB)
    Wb = W.reshape(nblk, NB, NB)
    assert np.all(np.isfinite(Wb))
    nbk = n - (nblk - 1) * NB
    last = Wb[-1]
    eye = np.eye(NB)
    assert np.array_equal(last[nbk:, :], eye[nbk:, :]) and np.array_equal(last[:, nbk:], eye[:, nbk:])


PLAIN = [c for c in CASES if c["kind"] != sc.COOP_FLAGS]


@pytest.mark.parametrize("case", PLAIN, ids=[c["id"] for c in PLAIN])
def test_substitution(ctx, case):
    ratio, Xs, Ls, Bs = run_case(ctx, case)
    print(f"{case['id']}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio
    if case["lower"] and case["count"] == 1:
        # the clipped solve agrees with the unclipped one on the same data
        X0, L0, _, _, _ = run_single(ctx, case, rhs_lower=0)
        assert np.array_equal(L0, Ls[0])
        b = sc.BLOCK_WIDTH[case["kind"]]
        assert sc.residual_ratio(L0, X0, Bs[0], b, False) <= 1.0
        agree = sc.agreement_ratio(L0, Xs[0], X0, Bs[0], b, False)
        print(f"{case['id']}: rhs_lower 1 against 0, difference / bound {agree:.3g}")
        assert agree <= 1.0, agree


FLAGS = [c for c in CASES if c["kind"] == sc.COOP_FLAGS]


@pytest.mark.parametrize("case", FLAGS, ids=[c["id"] for c in FLAGS])
def test_backward_solve_coop_flags(make_ctx, monkeypatch, case):
    """More than 16 blocks: per-block flags as the hand-over, which the product dispatches only under a raised
    AGP_BACKSUB_COOP_MAX (tests/test_fit_schedules_gpu.py: BS_COOP_FLAGS)."""
    monkeypatch.setenv("AGP_BACKSUB_COOP_MAX", "4096")
    ratio, _, _, _ = run_case(make_ctx(), case)
    print(f"{case['id']}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


ZERO_STRIDE = [(sc.FWD_MAT_BATCHED, sc.FWD_MAT, "forward_solve_mat", 129, 65), (sc.FWD_MAT_BATCHED, sc.FWD_MAT, "forward_solve_mat", 513, 64),
               (sc.RIGHT_LT_BATCHED, sc.RIGHT_LT, "right_solve_lt", 129, 65), (sc.BWD_VEC_BATCHED, sc.BWD_VEC, "backward_solve_vec", 129, 1),
               (sc.BWD_VEC_BATCHED, sc.BWD_VEC, "backward_solve_vec", 700, 1), (sc.COOP_BATCHED, sc.COOP_DIRECT, "backward_solve_coop", 513, 1)]


@pytest.mark.parametrize("bkind,skind,name,n,cols", ZERO_STRIDE, ids=[f"{z[2]}-{z[3]}-{z[4]}" for z in ZERO_STRIDE])
def test_batch_of_one_with_zero_strides_agrees_with_unbatched(ctx, bkind, skind, name, n, cols):
    bcase = sc.make_case(bkind, name + "_batched", n, cols, "gram")
    scase = sc.make_case(skind, name, n, cols, "gram")
    Xs, Ls, Bs, flags = run_batched(ctx, bcase, zero_strides=True)
    X1, L1, B1, _, _ = run_single(ctx, scase)
    assert np.array_equal(Ls[0], L1) and np.array_equal(Bs[0], B1)
    tr = bkind in sc.TRANSPOSED
    if bkind == sc.COOP_BATCHED:
        check_coop(flags, Xs)
    r0 = sc.residual_ratio(L1, Xs[0], B1, sc.BLOCK_WIDTH[bkind], tr)
    r1 = sc.residual_ratio(L1, X1, B1, sc.BLOCK_WIDTH[skind], tr)
    agree = sc.agreement_ratio(L1, Xs[0], X1, B1, sc.BLOCK_WIDTH[bkind], tr, b2=sc.BLOCK_WIDTH[skind])
    print(f"{name} n={n}: batched {r0:.3g}, unbatched {r1:.3g}, difference / bound {agree:.3g}")
    assert r0 <= 1.0 and r1 <= 1.0 and agree <= 1.0


@pytest.mark.parametrize("n,k0", sc.BACK_UPDATE_SHAPES)
@pytest.mark.parametrize("parity", ["odd", "even"])
@pytest.mark.parametrize("family", ["rand", "gram"])
def test_back_update(ctx, n, k0, parity, family):
    """back_update_kernel: z[c] -= sum_r L[k0 + r][c] x[r] for c < k0, at an odd (scalar loads) and an even (double2
    loads) leading dimension of the factor."""
    lda = sc.odd_even_lda(n)[0 if parity == "odd" else 1]
    z, x = sc.back_update_vectors(n, k0)
    M = np.zeros((k0, 2))
    M[:, 0] = z
    M[:len(x), 1] = x
    ldb = pick_ld(k0)
    flat, view = padded(M, ldb)
    st, _, Ls, _ = substitute(ctx, sc.BACK_UPDATE, [sc.spd_matrix(family, n)], flat, k0, 2, ldb, lda=lda, opt=k0)
    assert st == 0
    check_padding(flat, view, k0, 2)
    assert np.array_equal(view[:k0, 1], M[:, 1])  # x is read only
    ratio = sc.back_update_ratio(Ls[0], k0, z, x, view[:k0, 0].copy())
    print(f"back_update n={n} k0={k0} lda={lda}: error / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


def test_coop_refuses_what_the_product_does_not_dispatch(ctx):
    """The debug entry point is no way to launch backsub_coop_kernel outside its liveness argument: n above
    backsub_coop_max (2047 by default), the direct hand-over on more than 16 blocks, flags on 16 or fewer."""
    K = np.eye(2304)
    for kind, n in ((sc.COOP_DIRECT, 2048), (sc.COOP_FLAGS, 2304), (sc.COOP_BATCHED, 2304), (sc.COOP_FLAGS, 1000)):
        buf = np.zeros(n + 3)
        st, _, _, _ = substitute(ctx, kind, [K[:n, :n]], buf, n, 1, n + 3)
        assert st == INVALID_ARGUMENT, (kind, n, st)
        assert np.all(buf == 0.0)
