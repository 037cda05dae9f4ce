"""agp_pivoted_cholesky (csrc/pivoted_chol.hip) on the GPU: its own output against the matrix K = ctx.gram(cov, X), every
bound recomputed in longdouble from the returned L (tests/pivoted_chol_cases.py derives the bounds and names the shapes;
tests/test_pivoted_chol_host.py shows a float64 restatement meets them on these inputs).  Pivots are never compared with a
free-running reference.  Beyond the bounds each case asserts determinism (two calls, equal bits) and memory safety (the
NaN padding rows of ldl > n, the columns from rank on and pivots[rank:] untouched, bit for bit)."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import pivoted_chol_cases as pc

pytestmark = pytest.mark.gpu

PIVOT_FILL = -7777


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def call(ctx, cov, struct, n, max_rank, rel_tol, pad=3, want_l=True, want_resid=True, want_trace=True, location=capi.HOST,
         ldl=None):
    """the C-ABI call with NaN-filled host outputs; returns (status, pivots buffer, rank, L buffer (ldl x max_rank), resid,
    trace) as the call left them"""
    ldl = n + pad if ldl is None else ldl
    m = max(max_rank, 1)
    pivots = np.full(m, PIVOT_FILL, dtype=np.int64)
    rank = C.c_int64(PIVOT_FILL)
    Lbuf = np.full((max(ldl, 1), m), np.nan, order="F") if want_l else None
    resid = np.full(n, np.nan) if want_resid else None
    trace = C.c_double(np.nan)
    st = ctx._lib.agp_pivoted_cholesky(ctx._h, ctx.kernel(cov), C.byref(struct), max_rank, rel_tol, _p(pivots), C.byref(rank),
                                       _p(Lbuf), ldl, _p(resid), location, C.byref(trace) if want_trace else None)
    return st, pivots, int(rank.value), Lbuf, resid, trace.value


def host_struct(cov, x):
    fs = cov.features(x)
    return fs.as_struct(), fs


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_pivoted_cholesky_against_the_matrix(ctx, name):
    cov, x = pc.inputs(name)
    n, _, _, max_rank, rel_tol, _ = pc.CASES[name]
    s, keep = host_struct(cov, x)
    st, pivots, rank, Lbuf, resid, trace = call(ctx, cov, s, n, max_rank, rel_tol)
    assert st == capi.AGP_OK
    assert 0 <= rank <= max_rank
    # memory safety: padding rows, columns from rank on, pivots[rank:]
    assert np.all(np.isnan(Lbuf[n:, :])) and np.all(np.isnan(Lbuf[:, rank:]))
    assert np.all(pivots[rank:] == PIVOT_FILL)
    assert not np.any(np.isnan(Lbuf[:n, :rank])) and not np.any(np.isnan(resid)) and trace == trace
    kdiag, krows, _ = pc.gram_parts(ctx.gram, name, pivots[:rank])
    worst = pc.check(kdiag, krows, max_rank, rel_tol, pivots[:rank], rank, np.array(Lbuf[:n, :rank]), resid, trace)
    print(name, "rank", rank, worst)
    if name.startswith("duplicates"):
        assert rank == pc.DUPLICATE_RANK
        xs = pc.coords_of(x)
        assert len({xs[p].tobytes() for p in pivots[:rank]}) == rank, "two copies of one point were selected"
    elif name == "early_stop":
        assert 0 < rank < max_rank
    elif name == "ties":
        assert pivots[:rank].tolist() == [0], "equal values: the lowest index wins"
    else:
        assert rank == max_rank
    if name != "early_stop" and not name.startswith("duplicates") and rank:
        assert pivots[0] == int(np.flatnonzero(kdiag == kdiag.max())[0]), "step 0 picks the FIRST largest diagonal entry"
    # determinism: a second call, the same bits
    st2, pivots2, rank2, Lbuf2, resid2, trace2 = call(ctx, cov, s, n, max_rank, rel_tol)
    assert st2 == capi.AGP_OK and rank2 == rank and np.array_equal(pivots2, pivots)
    assert np.array_equal(_bits(Lbuf2), _bits(Lbuf)) and np.array_equal(_bits(resid2), _bits(resid))
    assert np.array([trace2]).view(np.uint64)[0] == np.array([trace]).view(np.uint64)[0]


@pytest.mark.parametrize("name", ["rows129", "noise_ids", "scaling"])
def test_locations_agree_bit_for_bit(ctx, name):
    """features on the host and on the device; L on the host, on the device (even and odd ldl: the 16-byte and the
    8-byte path of the column loads) and NULL: one result"""
    cov, x = pc.inputs(name)
    n, _, _, max_rank, rel_tol, _ = pc.CASES[name]
    fs = cov.features(x)
    s = fs.as_struct()
    st, pivots, rank, Lbuf, resid, trace = call(ctx, cov, s, n, max_rank, rel_tol, pad=0)
    assert st == capi.AGP_OK
    # no L, no residual, no trace
    st, pivots_n, rank_n, _, _, _ = call(ctx, cov, s, n, max_rank, rel_tol, want_l=False, want_resid=False, want_trace=False)
    assert st == capi.AGP_OK and rank_n == rank and np.array_equal(pivots_n, pivots)
    # features on the device
    dev = [ctx.to_device(fs.coords)]
    sd = capi.Features()
    sd.n, sd.dim, sd.n_scale_columns = fs.n, fs.dim, fs.n_scale_columns
    sd.coords = dev[0].ptr
    sd.eq_id = sd.scales = None
    if fs.eq_id is not None:
        dev.append(ctx.to_device(fs.eq_id))
        sd.eq_id = dev[-1].ptr
    if fs.scales is not None:
        dev.append(ctx.to_device(np.ascontiguousarray(fs.scales.T)))  # n x columns column-major = columns x n row-major
        sd.scales = dev[-1].ptr
    sd.is_measurement, sd.location = 0, capi.DEVICE
    st, pivots_d, rank_d, Lbuf_d, resid_d, trace_d = call(ctx, cov, sd, n, max_rank, rel_tol, pad=0)
    assert st == capi.AGP_OK and rank_d == rank and np.array_equal(pivots_d, pivots)
    assert np.array_equal(_bits(Lbuf_d), _bits(Lbuf)) and np.array_equal(_bits(resid_d), _bits(resid)) and trace_d == trace
    # L and the residual on the device, NaN-filled there first
    for ldl in (n + (n & 1), n + 1 - (n & 1)):  # even, odd
        Ld = ctx.to_device(np.full((ldl * max_rank,), np.nan))
        rd = ctx.to_device(np.full((n,), np.nan))
        piv = np.full(max_rank, PIVOT_FILL, dtype=np.int64)
        rk, tr = C.c_int64(-1), C.c_double(np.nan)
        st = ctx._lib.agp_pivoted_cholesky(ctx._h, ctx.kernel(cov), C.byref(sd), max_rank, rel_tol, _p(piv), C.byref(rk),
                                           C.c_void_p(Ld.ptr), ldl, C.c_void_p(rd.ptr), capi.DEVICE, C.byref(tr))
        assert st == capi.AGP_OK and rk.value == rank and np.array_equal(piv, pivots)
        got = Ld.numpy().reshape((ldl, max_rank), order="F")
        assert np.array_equal(_bits(got[:n, :rank]), _bits(Lbuf[:n, :rank]))
        assert np.all(np.isnan(got[n:, :])) and np.all(np.isnan(got[:, rank:]))
        assert np.array_equal(_bits(rd.numpy()), _bits(resid)) and tr.value == trace
        Ld.free()
        rd.free()
    for d in dev:
        d.free()


def test_python_surface(ctx):
    cov, x = pc.inputs("early_stop")
    n, _, _, max_rank, rel_tol, _ = pc.CASES["early_stop"]
    f = ab.pivoted_cholesky(cov, x, max_rank, rel_tol, context=ctx)
    assert f.factor.shape == (n, f.rank) and f.pivots.shape == (f.rank,) and 0 < f.rank < max_rank
    kdiag, krows, _ = pc.gram_parts(ctx.gram, "early_stop", f.pivots)
    pc.check(kdiag, krows, max_rank, rel_tol, f.pivots, f.rank, f.factor, f.residual_diagonal, f.trace_residual)
    g = ab.pivoted_cholesky(cov, x, max_rank, rel_tol, on_device=True, context=ctx)
    assert isinstance(g.factor, ab.DeviceArray) and g.rank == f.rank and np.array_equal(g.pivots, f.pivots)
    got = g.factor.numpy().ravel().reshape((n, max_rank), order="F")[:, :g.rank]
    assert np.array_equal(_bits(got), _bits(f.factor))
    assert np.array_equal(_bits(g.residual_diagonal.numpy()), _bits(f.residual_diagonal))
    h = ab.pivoted_cholesky(cov, x, 10 * n, 0.5, want_factor=False, context=ctx)  # max_rank is clipped to n
    assert h.factor is None and 0 < h.rank < f.rank and np.array_equal(h.pivots, f.pivots[:h.rank])
    with pytest.raises(ValueError):
        ab.pivoted_cholesky(cov, [ab.LinearCombination([x[0], x[1]])], 1, context=ctx)


def test_profiling_stage(ctx):
    cov, x = pc.inputs("rows257")
    ctx.set_profiling(True)
    try:
        ab.pivoted_cholesky(cov, x, 24, context=ctx)
        assert ctx.stage_ms(10) > 0.
    finally:
        ctx.set_profiling(False)


@pytest.mark.parametrize("what", ["max_rank_0", "max_rank_above_n", "negative_tol", "nan_tol", "short_ldl", "bad_location",
                                  "null_pivots", "null_rank"])
def test_invalid_arguments_write_nothing(ctx, what):
    cov, x = pc.inputs("rows129")
    n = 129
    s, keep = host_struct(cov, x)
    kw = dict(max_rank=8, rel_tol=0., location=capi.HOST, ldl=n + 3)
    kw.update({"max_rank_0": dict(max_rank=0), "max_rank_above_n": dict(max_rank=n + 1), "negative_tol": dict(rel_tol=-1e-300),
               "nan_tol": dict(rel_tol=float("nan")), "short_ldl": dict(ldl=n - 1), "bad_location": dict(location=2),
               "null_pivots": {}, "null_rank": {}}[what])
    m = max(kw["max_rank"], 1)
    pivots = np.full(m, PIVOT_FILL, dtype=np.int64)
    rank, trace = C.c_int64(PIVOT_FILL), C.c_double(np.nan)
    Lbuf = np.full((n + 3, m), np.nan, order="F")
    resid = np.full(n, np.nan)
    st = ctx._lib.agp_pivoted_cholesky(ctx._h, ctx.kernel(cov), C.byref(s), kw["max_rank"], kw["rel_tol"],
                                       None if what == "null_pivots" else _p(pivots), None if what == "null_rank" else C.byref(rank),
                                       _p(Lbuf), kw["ldl"], _p(resid), kw["location"], C.byref(trace))
    assert st == capi.AGP_ERR_INVALID_ARGUMENT
    assert np.all(pivots == PIVOT_FILL) and rank.value == PIVOT_FILL and trace.value != trace.value
    assert np.all(np.isnan(Lbuf)) and np.all(np.isnan(resid))


@pytest.mark.parametrize("row", [0, 200])
def test_nan_coordinate_is_reported(ctx, row):
    cov, x = pc.inputs("rows257")
    bad = np.array(x)
    bad[row, 1] = np.nan
    s, keep = host_struct(cov, bad)
    st, pivots, rank, _, _, _ = call(ctx, cov, s, 257, 24, 0.)
    assert st == capi.AGP_ERR_NAN_INPUT
    assert np.all(pivots == PIVOT_FILL) and rank == PIVOT_FILL
    with pytest.raises(ab.NanInputError):
        ab.pivoted_cholesky(cov, bad, 24, context=ctx)
