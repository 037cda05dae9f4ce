"""The column-pivoted Householder QR of csrc/qr.hip and the substitutions against its R factor, each on its own through
the agp_debug_colpiv_qr / qr_extract_r / qr_root / qr_sqrt_solve / qr_back_solve entry points (csrc/debug_api.hip), at
the edges of their 256- and 1024-wide strided loops and of the 64-wide blocks of the R^T solve.

Shapes, inputs, the numpy restatement that serves as reference and every bound are tests/qr_cases.py's (its docstring
derives them; tests/test_qr_bounds_host.py shows the restatement in float64 meets them on these very inputs).  Each case
asserts the pivots, the backward and forward bounds as ratio <= 1, the counts in `state`, and memory safety bit for
bit: the NaN padding rows of lda > rows, the NaN columns behind cols + extra, the NaN rows of R, X and W beyond m."""
import ctypes as C

import numpy as np
import pytest

from albatross_amd import _capi as capi
import qr_cases as qc

pytestmark = pytest.mark.gpu

NAN_BITS = np.array(np.nan).view(np.uint64)
INVALID_ARGUMENT = 1  # include/albatross_amd.h: AGP_ERR_INVALID_ARGUMENT
EXTRA_COLS = 2
CASES = qc.qr_cases()


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def padded(M, ld, extra_cols=EXTRA_COLS):
    """M (rows x cols) in a NaN-filled column-major buffer of leading dimension ld with extra_cols further columns."""
    rows, cols = M.shape
    buf = np.full((ld, cols + extra_cols), np.nan, order="F")
    buf[:rows, :cols] = M
    return buf


def check_padding(buf, rows, cols):
    assert np.all(_bits(buf[rows:, :]) == NAN_BITS), "padding rows written"
    assert np.all(_bits(buf[:, cols:]) == NAN_BITS), "columns beyond the matrix written"


def colpiv_qr(ctx, M, cols, extra, lda=None, alloc_cols=None):
    """agp_debug_colpiv_qr on [A | y] = M: (status, padded buffer, tau, perm, state)."""
    rows = M.shape[0]
    buf = padded(M, qc.pick_ld(rows))
    tau = np.full(cols, np.nan)
    perm = np.full(cols, -1, dtype=np.int64)
    state = np.full(4, np.nan)
    st = capi.load_debug().agp_debug_colpiv_qr(ctx._h, _p(buf), buf.shape[0] if lda is None else lda, rows, cols, extra,
                                               buf.shape[1] if alloc_cols is None else alloc_cols, _p(tau), _p(perm), _p(state))
    return st, buf, tau, perm, state


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_colpiv_qr(ctx, case):
    name, extra = case["name"], case["extra"]
    A, y, det = qc.qr_input(name)
    rows, cols = A.shape
    ref = qc.restated(name, "ref")
    st, buf, tau, perm, state = colpiv_qr(ctx, np.column_stack([A] + ([y] if extra else [])), cols, extra)
    assert st == 0, st
    check_padding(buf, rows, cols + extra)
    qr = buf[:rows, :cols + extra].copy()
    assert np.all(np.isfinite(qr)) and np.all(np.isfinite(tau))
    # the pivots
    assert sorted(perm) == list(range(cols))
    assert np.array_equal(perm[:det], ref["perm"][:det]), np.flatnonzero(perm[:det] != ref["perm"][:det])[:5]
    # the bounds
    t = qc.tau_ratio(qr, tau, cols)
    b = qc.backward_ratio(name, extra, qr, tau, perm)
    fw, below = qc.forward_ratios(name, extra, qr, perm)
    print(f"{case['id']}: tau {t:.3g}, backward {b:.3g}, forward {fw:.3g}, below the determined rows {below:.3g}")
    assert t <= 1.0, t
    assert b <= 1.0, b
    assert fw <= 1.0, fw
    assert below <= 1.0, below
    # the counts (state[0]: the initial norms of qr_norms_kernel, which otherwise only choose the first pivot)
    h = qc.helper_ratio(name, state[0])
    assert h <= 1.0, h
    assert state[1] == np.abs(np.diagonal(qr)[:cols]).max()
    assert state[3] == ref["rank"], (state[3], ref["rank"])
    if name not in qc.NP_EXEMPT:
        assert state[2] == ref["nonzero_pivots"], (state[2], ref["nonzero_pivots"])
    # what each special case is there for
    if name == "zeros":
        assert state[2] == 20 and state[3] == 20
        assert np.all(_bits(tau[20:]) == 0) and np.all(_bits(np.triu(qr[:cols, :cols])[20:, 20:]) == 0)
        assert np.all(qr[20:, 20:cols] == 0.0)
        # no swap among all-zero norms, the first index wins each tie: perm[20:] is what the first 20 swaps left there
        assert np.array_equal(perm, qc.after_swaps(perm, 20)) and np.array_equal(perm, ref["perm"])
    if name == "zerocol":
        assert perm[11] == 5 and state[2] == 11 and state[3] == 11 and tau[11] == 0.0 and np.all(qr[11:, 11] == 0.0)
    if name == "tie":
        assert perm[0] == 2
    if name == "lowrank":
        assert state[3] == qc.LOWRANK[1]


def test_colpiv_qr_refuses_what_the_product_never_asks(ctx):
    """rows < cols (qr_extract_r would read outside the rows), lda < rows, alloc_cols < cols + extra: refused, and
    nothing is written."""
    rng = np.random.default_rng(1)
    for rows, cols, extra, lda, alloc in ((5, 6, 0, None, None), (6, 5, 1, 5, None), (6, 5, 1, None, 5), (6, 5, 0, None, 4)):
        M = rng.standard_normal((rows, cols + extra))
        st, buf, tau, perm, state = colpiv_qr(ctx, M, cols, extra, lda=lda, alloc_cols=alloc)
        assert st == INVALID_ARGUMENT, (rows, cols, extra, lda, alloc, st)
        assert np.array_equal(buf[:rows, :cols + extra], M)
        check_padding(buf, rows, cols + extra)
        assert np.all(np.isnan(tau)) and np.all(perm == -1) and np.all(np.isnan(state))


COPY_SIZES = [1, 64, 257, 300]  # one and two blocks of 256 rows per column


@pytest.mark.parametrize("inflate", [0.0, 1e-10])
@pytest.mark.parametrize("m", COPY_SIZES)
def test_qr_extract_r(ctx, m, inflate):
    rng = np.random.default_rng(70 + m)
    A = padded(rng.standard_normal((m + 5, m)), qc.pick_ld(m + 5), extra_cols=0)  # a factored matrix has rows below m
    R = np.full((qc.pick_ld(m) + 1, m), np.nan, order="F")
    st = capi.load_debug().agp_debug_qr_extract_r(ctx._h, _p(A), A.shape[0], m, _p(R), R.shape[0], inflate)
    assert st == 0, st
    want = np.triu(A[:m, :m])
    want[np.diag_indices(m)] = np.diagonal(A)[:m] + inflate  # fl(a_ii + inflate)
    assert np.array_equal(_bits(R[:m]), _bits(want)), "upper triangle, inflated diagonal, +0 below"
    assert np.all(_bits(R[m:]) == NAN_BITS), "rows beyond m written"


@pytest.mark.parametrize("m", COPY_SIZES)
def test_qr_root(ctx, m):
    """T = P R^T: T[perm[i], r] = R[r, i], every other entry of the ldt x m buffer +0, with ldt > m."""
    rng = np.random.default_rng(80 + m)
    R = padded(np.triu(rng.standard_normal((m, m))), qc.pick_ld(m), extra_cols=0)
    perm = rng.permutation(m).astype(np.int64)
    T = np.full((m + 5, m), np.nan, order="F")
    st = capi.load_debug().agp_debug_qr_root(ctx._h, _p(R), R.shape[0], _p(perm), m, _p(T), T.shape[0])
    assert st == 0, st
    want = np.zeros_like(T)
    want[perm, :] = R[:m, :m].T
    assert np.array_equal(_bits(T), _bits(want))


def test_qr_entry_points_refuse_a_bad_permutation(ctx):
    m = 6
    R = np.asfortranarray(np.triu(np.ones((m, m))))
    T = np.full((m, m), np.nan, order="F")
    for bad in ([0, 1, 2, 3, 4, 6], [0, 1, 2, 3, 4, -1], [0, 1, 2, 3, 4, 4]):
        perm = np.array(bad, dtype=np.int64)
        assert capi.load_debug().agp_debug_qr_root(ctx._h, _p(R), m, _p(perm), m, _p(T), m) == INVALID_ARGUMENT
        assert np.all(_bits(T) == NAN_BITS)


@pytest.mark.parametrize("m,nrhs", qc.SQRT_SHAPES)
def test_qr_sqrt_solve(ctx, m, nrhs):
    R0, perm = qc.square_factor(m)
    X0 = qc.solve_rhs(m, nrhs)
    ldr, ldx, ldw = m + 1, m + 2, m + 3  # pairwise different, each > m
    R = padded(R0, ldr, extra_cols=0)
    X = padded(X0, ldx)
    W = np.full((ldw, nrhs + EXTRA_COLS), np.nan, order="F")
    Xbits = _bits(X).copy()
    perm = np.ascontiguousarray(perm)
    st = capi.load_debug().agp_debug_qr_sqrt_solve(ctx._h, _p(R), ldr, _p(perm), m, _p(X), ldx, _p(W), ldw, nrhs, W.shape[1])
    assert st == 0, st
    assert np.array_equal(_bits(X), Xbits), "X is read only"
    check_padding(W, m, nrhs)
    got = W[:m, :nrhs].copy()
    assert np.all(np.isfinite(got))
    ratio = qc.sqrt_solve_ratio(R0, perm, X0, got)
    print(f"sqrt_solve m={m} nrhs={nrhs}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("m,npv", qc.BACK_SHAPES)
def test_qr_back_solve(ctx, m, npv):
    R0, perm = qc.square_factor(m)
    c0 = qc.solve_rhs(m, 1)[:, 0]
    R = padded(R0, qc.pick_ld(m), extra_cols=0)
    c = np.concatenate([c0, [np.nan, np.nan]])
    out = np.full(m + 2, np.nan)
    perm = np.ascontiguousarray(perm)
    st = capi.load_debug().agp_debug_qr_back_solve(ctx._h, _p(R), R.shape[0], _p(perm), m, npv, _p(c), _p(out))
    assert st == 0, st
    assert np.all(_bits(c[m:]) == NAN_BITS) and np.all(_bits(out[m:]) == NAN_BITS), "a store past the end"
    assert np.array_equal(_bits(c[npv:m]), _bits(c0[npv:])), "c beyond np written"
    z = c[:npv].copy()
    assert np.array_equal(_bits(out[perm[:npv]]), _bits(z)), "the scatter through perm is exact"
    assert np.all(_bits(out[perm[npv:]]) == 0), "out[perm[i]] = +0 for i >= np"
    ratio = qc.back_solve_ratio(R0, npv, c0, z)
    print(f"back_solve m={m} np={npv}: residual / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio
