"""agp_gram_matvec (csrc/gram_matvec.hip) on the GPU against the matrix K = ctx.gram(cov, x): the bound and the shapes of
tests/gram_matvec_cases.py (tests/test_gram_matvec_host.py shows a float64 restatement meets the bound on these inputs).
Every case asserts the evaluator the dispatcher chose first (agp_debug_gram_matvec_plan); entry parity - columns of the
identity give the columns of the matrix bit for bit - pins "the same bits as agp_gram" on every path."""
import ctypes as C

import numpy as np
import pytest

import albatross_amd as ab
from albatross_amd import _capi as capi
import gram_matvec_cases as mc

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def matrix(ctx, cov, fs, y_var):
    return mc.system_matrix(ctx.gram(cov, mc.gram_argument(fs)), y_var)


def test_constants_and_slice_rule(ctx):
    """the constants the cases file names are the kernel's, and its slice rule is the library's"""
    cov = mc.gp.fast_cov(0, "noise")
    for n in mc.SIZES + [4096, 5000]:
        fs = mc.make_features(cov, mc.points(n, 3, 1), False, False)
        for nrhs in mc.NRHS:
            p = mc.plan(ctx, cov, fs, nrhs)
            assert p[0] == mc.FAST and tuple(p[1:3]) == mc.slices(n), (n, p)
            assert p[3:5] == [mc.MV_ROWS, mc.MV_COLS] and p[5] == mc.chunk_widths(nrhs)[0][0]
    assert mc.slices(mc.LARGEST_UNSPLIT)[0] == 1 and mc.slices(mc.FIRST_SPLIT)[0] == 2
    assert ab.MATVEC_MAX_RHS == mc.MV_MAX_RHS


@pytest.mark.parametrize("n", mc.SIZES)
def test_shapes_against_the_matrix(ctx, n):
    """every nrhs at every size: the bound, padded leading dimensions with canaries, y_var given, determinism"""
    cov = mc.gp.fast_cov(0, "noise")
    fs = mc.make_features(cov, mc.points(n, 3, 11 + n), False, False)
    y_var = mc.variances(n, n)
    Am = matrix(ctx, cov, fs, y_var)
    worst = 0.
    for k, nrhs in enumerate(mc.NRHS):
        V = mc.right_hand_sides(n, nrhs, 100 * n + nrhs)
        ldv, ldo = (n, n) if k % 2 == 0 else (n + 3, n + 5)
        st, out, pad, beyond = mc.call(ctx, cov, fs, V, y_var, ldv=ldv, ldo=ldo, extra_cols=2)
        assert st == capi.AGP_OK
        assert mc.all_canary(pad) and mc.all_canary(beyond), "a store outside the n x nrhs block"
        ok, frac = mc.within_bound(np.array(out), Am, V)
        assert ok, (n, nrhs, frac)
        worst = max(worst, frac)
        st2, out2, _, _ = mc.call(ctx, cov, fs, V, y_var, ldv=ldv, ldo=ldo, extra_cols=2)
        assert st2 == capi.AGP_OK and np.array_equal(_bits(out2), _bits(out)), "two calls, different bits"
    print(n, "slices", mc.slices(n), "worst fraction of the bound", worst)


@pytest.mark.parametrize("n", [65, 257, 513])
def test_entry_parity_all_columns(ctx, n):
    """the whole identity in chunks of every width: out is the matrix agp_gram gives, bit for bit, y_var on the diagonal"""
    cov = mc.gp.fast_cov(2, "noise")
    fs = mc.make_features(cov, mc.points(n, 2, n), False, False)
    for y_var in (None, mc.variances(n, 2)):
        Am = matrix(ctx, cov, fs, y_var)
        first, widths = 0, [33, 16, 3, 1, 17, 8, 15, 2]
        k = 0
        while first < n:
            w = min(widths[k % len(widths)], n - first)
            st, out, _, _ = mc.call(ctx, cov, fs, mc.identity_block(n, first, w), y_var)
            assert st == capi.AGP_OK
            assert np.array_equal(np.array(out), Am[:, first:first + w]), (n, first, w)
            first += w
            k += 1


@pytest.mark.parametrize("name,dim", mc.tree_cases())
def test_every_path(ctx, name, dim):
    """each tree on the evaluator it must take: measurement and plain features, with and without ids, y_var NULL and given"""
    cov, want_path = mc.tree(name)
    n = mc.PATH_N
    x = mc.points(n, dim, 7 * dim + len(name))
    for k, (meas, ids) in enumerate(mc.FEATURE_VARIANTS):
        fs = mc.make_features(cov, x, meas, ids)
        p = mc.plan(ctx, cov, fs, mc.PATH_NRHS)
        assert p[0] == want_path, (name, dim, mc.PATH_NAMES[p[0]])
        assert tuple(p[1:3]) == mc.slices(n)
        y_var = mc.variances(n, 3) if k % 2 == 0 else None
        Am = matrix(ctx, cov, fs, y_var)
        V = mc.right_hand_sides(n, mc.PATH_NRHS, 31 + k)
        st, out, _, _ = mc.call(ctx, cov, fs, V, y_var)
        assert st == capi.AGP_OK
        ok, frac = mc.within_bound(np.array(out), Am, V)
        assert ok, (name, dim, meas, ids, frac)
        # entry parity: the last 17 columns (the ragged tile of the last slice, the duplicate of point 0 among them) and
        # the first 16
        for first, w in ((n - mc.PATH_NRHS, mc.PATH_NRHS), (0, 16)):
            st, got, _, _ = mc.call(ctx, cov, fs, mc.identity_block(n, first, w), y_var)
            assert st == capi.AGP_OK
            assert np.array_equal(np.array(got), Am[:, first:first + w]), (name, dim, meas, ids, first)


def test_interpreter_when_the_structured_evaluators_are_off(make_ctx, monkeypatch):
    """AGP_GRAM_SOP=0: every tree on the postfix interpreter, still the bits of agp_gram under the same switch"""
    monkeypatch.setenv("AGP_GRAM_SOP", "0")
    c = make_ctx()
    n = 130
    for cov in (mc.gp.fast_cov(3, "noise"), mc.gp.generic_noise_cov()):
        fs = mc.make_features(cov, mc.points(n, 3, 4), True, False)
        assert mc.plan(c, cov, fs)[0] == mc.INTERP
        Am = matrix(c, cov, fs, None)
        st, got, _, _ = mc.call(c, cov, fs, mc.identity_block(n, n - 16, 16))
        assert st == capi.AGP_OK and np.array_equal(np.array(got), Am[:, n - 16:])


def test_device_location_and_python_surface(ctx):
    """x, y_var, V and out on the device give the bits of the host call; ab.gram_matvec on both"""
    n, nrhs = 513, 17
    cov = mc.gp.fast_cov(1, "noise")
    x = mc.points(n, 3, 9)
    fs = mc.make_features(cov, x, False, False)
    y_var = mc.variances(n, 1)
    V = mc.right_hand_sides(n, nrhs, 2)
    st, want, _, _ = mc.call(ctx, cov, fs, V, y_var)
    assert st == capi.AGP_OK
    host = ab.gram_matvec(cov, x, V, y_var, context=ctx)
    assert np.array_equal(_bits(host), _bits(want))
    one = ab.gram_matvec(cov, x, V[:, 0].copy(), y_var, context=ctx)
    assert one.shape == (n,)
    ok, _ = mc.within_bound(one.reshape(n, 1), matrix(ctx, cov, fs, y_var), V[:, :1])
    assert ok
    # device: a padded out block (ldo = n + 3, two columns beyond nrhs) full of canaries
    dc = ctx.to_device(fs.coords)
    s = capi.Features()
    s.n, s.dim, s.n_scale_columns, s.coords, s.eq_id, s.scales = n, 3, 0, dc.ptr, None, None
    s.is_measurement, s.location = 0, capi.DEVICE
    dvar, dV = ctx.to_device(y_var), ctx.to_device(V.T.copy())  # (n, nrhs) column-major = (nrhs, n) row-major
    ldo = n + 3
    dout = ctx.to_device(mc.canaries(ldo * (nrhs + 2)))
    st = ctx._lib.agp_gram_matvec(ctx._h, ctx.kernel(cov), C.byref(s), C.c_void_p(dvar.ptr), C.c_void_p(dV.ptr), n, nrhs,
                                  C.c_void_p(dout.ptr), ldo, capi.DEVICE)
    assert st == capi.AGP_OK
    ob = dout.numpy().reshape(ldo, nrhs + 2, order="F")
    assert np.array_equal(_bits(ob[:n, :nrhs]), _bits(want))
    assert mc.all_canary(ob[n:]) and mc.all_canary(ob[:, nrhs:])
    dV.shape = (n, nrhs)  # the DeviceArray as ab.gram_matvec takes it: n x columns, its bytes column-major
    dres = ab.gram_matvec(cov, s, dV, dvar, on_device=True, context=ctx)
    got = dres.numpy().reshape(-1).reshape(n, nrhs, order="F")
    assert np.array_equal(_bits(got), _bits(want))


def test_invalid_arguments_write_nothing(ctx):
    n, nrhs = 65, 3
    cov = mc.gp.fast_cov(0, "none")
    fs = mc.make_features(cov, mc.points(n, 2, 3), False, False)
    s = fs.as_struct()
    V = mc.right_hand_sides(n, nrhs, 1)
    out = mc.canaries(n * nrhs)
    lib, kh = ctx._lib, ctx.kernel(cov)
    pV, po = C.c_void_p(V.ctypes.data), C.c_void_p(out.ctypes.data)
    bad = [
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n, 0, po, n, capi.HOST),       # nrhs < 1
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n, -2, po, n, capi.HOST),
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n - 1, nrhs, po, n, capi.HOST),  # ldv < n
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n, nrhs, po, n - 1, capi.HOST),  # ldo < n
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n, nrhs, po, n, 2),              # no such location
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n, nrhs, po, n, -1),
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, None, n, nrhs, po, n, capi.HOST),
        lib.agp_gram_matvec(ctx._h, kh, C.byref(s), None, pV, n, nrhs, None, n, capi.HOST),
        lib.agp_gram_matvec(ctx._h, kh, None, None, pV, n, nrhs, po, n, capi.HOST),
    ]
    assert bad == [capi.AGP_ERR_INVALID_ARGUMENT] * len(bad)
    assert mc.all_canary(out)


@pytest.mark.parametrize("name", ["fast_se_noise", "sop_generic_noise", "interp_sum_in_product"])
def test_nan_coordinate(ctx, name):
    n = 300
    cov, _ = mc.tree(name)
    x = mc.points(n, 3, 8)
    x[n - 2, 1] = np.nan
    fs = mc.make_features(cov, x, False, False)
    st, out, _, _ = mc.call(ctx, cov, fs, mc.right_hand_sides(n, 2, 1))
    assert st == capi.AGP_ERR_NAN_INPUT
    assert mc.all_canary(out), "a host block is not written when the call fails"
    with pytest.raises(ab.NanInputError):
        ab.gram_matvec(cov, x, np.ones(n), context=ctx)
